/* The sparse consumer from plain C: the Jacobian of a built-in 5-point family through a CSC plan, left on the device, then
 * (I - gamma J) y = b solved on the stored nzval by fd_csc_solve_async; prints the status and the true residual.
 *
 *   gcc -O2 -Iinclude examples/csc_solve_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fdjac.h"

extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t size, int kind); /* 1 = host->device, 2 = device->host */

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
    const int64_t nx = 96, ny = 80, N = nx * ny;
    /* the 5-point pattern as Julia stores it (1-based, rows ascending) and its five-colour distance-2 colouring */
    int64_t *colptr = malloc(sizeof(int64_t) * (size_t)(N + 1)), *rowval = malloc(sizeof(int64_t) * (size_t)(5 * N));
    int64_t *colors = malloc(sizeof(int64_t) * (size_t)N), nnz = 0;
    for (int64_t k = 0; k < N; ++k) {
        const int64_t i = k % nx, j = k / nx;
        colptr[k] = nnz + 1;
        if (j > 0) rowval[nnz++] = k - nx + 1;
        if (i > 0) rowval[nnz++] = k;
        rowval[nnz++] = k + 1;
        if (i < nx - 1) rowval[nnz++] = k + 2;
        if (j < ny - 1) rowval[nnz++] = k + nx + 1;
        colors[k] = (i + 2 * j) % 5 + 1;
    }
    colptr[N] = nnz + 1;
    double *x = malloc(sizeof(double) * (size_t)N), *b = malloc(sizeof(double) * (size_t)N);
    for (int64_t k = 0; k < N; ++k) { x[k] = 0.5 + 0.25 * sin((double)(k + 1)); b[k] = cos(0.37 * (double)k); }

    fd_ctx *ctx;
    CHECK(fd_ctx_create(0, NULL, &ctx));
    void *xd, *bd, *yd, *nzd;
    if (hipMalloc(&xd, sizeof(double) * (size_t)N) || hipMalloc(&bd, sizeof(double) * (size_t)N) || hipMalloc(&yd, sizeof(double) * (size_t)N) ||
        hipMalloc(&nzd, sizeof(double) * (size_t)nnz)) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    hipMemcpy(xd, x, sizeof(double) * (size_t)N, 1);
    hipMemcpy(bd, b, sizeof(double) * (size_t)N, 1);

    /* the Jacobian: forward differences of the built-in non-linear 5-point family, stored as SparseMatrixCSC nzval on the device */
    fd_f_launch f; void *fctx; fd_plan *plan;
    const int64_t prm[2] = {nx, ny};
    CHECK(fd_builtin_f_create(ctx, FD_F_LAP5_NL, prm, 2, &f, &fctx));
    fd_plan_opts o; memset(&o, 0, sizeof o); o.fdtype = FD_FORWARD;
    CHECK(fd_plan_create_csc(ctx, N, N, colptr, rowval, 8, 1, colors, 8, &o, &plan));
    void *outs[3] = {nzd, NULL, NULL};
    CHECK(fd_jacobian_async(plan, f, fctx, xd, NULL, -1.0, -1.0, 1.0, outs));

    /* the consumer, on the same stream: no synchronisation in between */
    const double gamma = 0.1;                  /* |J_ii| ~ 4, four neighbours ~ 1: I - gamma J is strictly dominant */
    fd_csc_solver *solver;
    CHECK(fd_csc_solver_create(ctx, N, colptr, rowval, 8, 1, FD_HOST, &solver));
    CHECK(fd_csc_solver_set_options(solver, 1e-12, 100));
    CHECK(fd_csc_solve_async(solver, 1.0, -gamma, nzd, bd, yd));
    int flags = -1; int64_t iters = -1; double resid = 0, bnorm = 0;
    CHECK(fd_csc_solver_status(solver, &flags, &iters, &resid, &bnorm));

    /* the true residual of (I - gamma J) y = b from the downloaded values */
    double *nz = malloc(sizeof(double) * (size_t)nnz), *y = malloc(sizeof(double) * (size_t)N), *r = malloc(sizeof(double) * (size_t)N);
    hipMemcpy(nz, nzd, sizeof(double) * (size_t)nnz, 2);
    hipMemcpy(y, yd, sizeof(double) * (size_t)N, 2);
    for (int64_t k = 0; k < N; ++k) r[k] = y[k] - b[k];
    for (int64_t k = 0; k < N; ++k)
        for (int64_t q = colptr[k] - 1; q < colptr[k + 1] - 1; ++q) r[rowval[q] - 1] -= gamma * nz[q] * y[k];
    double worst = 0;
    for (int64_t k = 0; k < N; ++k) if (!(fabs(r[k]) <= worst)) worst = fabs(r[k]);
    printf("csc solve: N = %lld nnz = %lld status %d iterations %lld ||r|| / ||b|| = %.3e  max|W y - b| = %.3e\n", (long long)N, (long long)nnz,
           flags, (long long)iters, bnorm > 0 ? resid / bnorm : 0.0, worst);
    const int ok = flags == 0 && worst <= 1e-9;

    CHECK(fd_csc_solver_destroy(solver));
    CHECK(fd_plan_destroy(plan));
    CHECK(fd_builtin_f_destroy(fctx));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(xd); hipFree(bd); hipFree(yd); hipFree(nzd);
    free(colptr); free(rowval); free(colors); free(x); free(b); free(nz); free(y); free(r);
    return ok ? 0 : 3;
}
