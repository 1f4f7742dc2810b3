/* The sparse consumer's warm start from plain C: an implicit-step sequence (I - gamma J) u+ = u on the 5-point pattern, every step
 * solved cold (fd_csc_solve_async) and from the first-order guess y0 = b = u (fd_csc_solve_from_async), device pointers through the
 * boundary.  J = diag(c) * (5-point Laplacian) on a 12 x 11 grid with c = 1 in the 6 x 6 corner and 1e-4 elsewhere, gamma = 100, and a
 * first state that is zero on the corner and its rim: the operator of tests/warm_cases.py, where the guess saves an iteration or two
 * of sixteen at most steps (on a homogeneous Laplacian it saves none: the stopping rule is relative to ||b||).  Prints both iteration
 * counts per step and the largest difference of the two solutions; the state follows the cold solves.
 *
 *   gcc -O2 -Iinclude examples/csc_warm_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fdjac.h"

extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t size, int kind); /* 1 = host->device, 2 = device->host, 3 = device->device */

#define CHECK(call)                                                                                \
    do {                                                                                           \
        int rc_ = (call);                                                                          \
        if (rc_ != 0) {                                                                            \
            fprintf(stderr, "%s:%d %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, fd_last_error()); \
            return rc_;                                                                            \
        }                                                                                          \
    } while (0)

int main(void)
{
    const int64_t nx = 12, ny = 11, N = nx * ny, corner = 6;
    const int steps = 4;
    const double gamma = 100.0, rtol = 1e-10;
    const size_t bytes = sizeof(double) * (size_t)N;
    int64_t *colptr = malloc(sizeof(int64_t) * (size_t)(N + 1)), *rowval = malloc(sizeof(int64_t) * (size_t)(5 * N)), nnz = 0;
    double *nz = malloc(sizeof(double) * (size_t)(5 * N)), *u = malloc(bytes), *yc = malloc(bytes), *yw = malloc(bytes);
    for (int64_t k = 0; k < N; ++k) {          /* column k, 0-based, rows ascending; entry (r, k) = c_r * (-4 on the diagonal, 1 off it) */
        const int64_t i = k % nx, j = k / nx;
        const int64_t rows[5] = {j > 0 ? k - nx : -1, i > 0 ? k - 1 : -1, k, i < nx - 1 ? k + 1 : -1, j < ny - 1 ? k + nx : -1};
        colptr[k] = nnz;
        for (int q = 0; q < 5; ++q) {
            const int64_t r = rows[q];
            if (r < 0) continue;
            const double c = (r % nx < corner && r / nx < corner) ? 1.0 : 1e-4;
            rowval[nnz] = r;
            nz[nnz++] = (r == k ? -4.0 : 1.0) * c;
        }
        u[k] = (i < corner + 1 && j < corner + 1) ? 0.0 : (double)((k * 37 + 11) % 101) / 50.0 - 1.0;
    }
    colptr[N] = nnz;

    fd_ctx *ctx;
    CHECK(fd_ctx_create(0, NULL, &ctx));
    void *ud, *ycd, *ywd, *nzd;
    if (hipMalloc(&ud, bytes) || hipMalloc(&ycd, bytes) || hipMalloc(&ywd, bytes) || hipMalloc(&nzd, sizeof(double) * (size_t)nnz)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    if (hipMemcpy(ud, u, bytes, 1) || hipMemcpy(nzd, nz, sizeof(double) * (size_t)nnz, 1)) return 1;
    fd_csc_solver *solver;
    CHECK(fd_csc_solver_create(ctx, N, colptr, rowval, 8, 0, FD_HOST, &solver));
    CHECK(fd_csc_solver_set_options(solver, rtol, 500));

    double worst = 0.0;
    int ok = 1;
    for (int s = 0; s < steps; ++s) {
        int fc = -1, fw = -1;
        int64_t ic = -1, iw = -1;
        CHECK(fd_csc_solve_async(solver, 1.0, -gamma, nzd, ud, ycd));
        CHECK(fd_csc_solver_status(solver, &fc, &ic, NULL, NULL));
        CHECK(fd_csc_solve_from_async(solver, 1.0, -gamma, nzd, ud, ud, ywd));          /* y0 is b */
        CHECK(fd_csc_solver_status(solver, &fw, &iw, NULL, NULL));
        if (hipMemcpy(yc, ycd, bytes, 2) || hipMemcpy(yw, ywd, bytes, 2)) return 1;
        for (int64_t k = 0; k < N; ++k)
            if (!(fabs(yw[k] - yc[k]) <= worst)) worst = fabs(yw[k] - yc[k]);
        printf("csc warm: step %d: cold status %d iterations %lld, warm status %d iterations %lld\n", s + 1, fc, (long long)ic, fw, (long long)iw);
        ok = ok && fc == 0 && fw == 0;
        if (hipMemcpy(ud, ycd, bytes, 3)) return 1;          /* the next step's u */
    }
    printf("csc warm: max |y_warm - y_cold| = %.17g\n", worst);
    ok = ok && worst <= 1e-8;          /* both within rtol ||b|| of the one solution; ||A^-1|| <= 1 */
    CHECK(fd_csc_solver_destroy(solver));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(ud); hipFree(ycd); hipFree(ywd); hipFree(nzd);
    free(colptr); free(rowval); free(nz); free(u); free(yc); free(yw);
    printf("csc warm: %s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
