/* Restarted GMRES beside BiCGStab from plain C, on the system BiCGStab cannot solve: N = 2 k, one stored entry per 2-block,
 * J[2i, 2i + 1] = 2, so every block of A = I + J is [[1, 2], [0, 1]]; b = (1, -1, 1, -1, ...).  BiCGStab's first rhat . v is an exact
 * zero (status 2, y = NaN); fd_csc_solver_set_method(solver, FD_CSC_METHOD_GMRES, 30) on the same handle solves it in two iterations:
 * y = (3, -1, 3, -1, ...).  Prints both status words.
 *
 *   gcc -O2 -Iinclude examples/csc_gmres_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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
    const int64_t k = 1025, N = 2 * k;
    int64_t *colptr = malloc(sizeof(int64_t) * (size_t)(N + 1)), *rowval = malloc(sizeof(int64_t) * (size_t)k);
    double *nz = malloc(sizeof(double) * (size_t)k), *b = malloc(sizeof(double) * (size_t)N), *y = malloc(sizeof(double) * (size_t)N);
    for (int64_t j = 0; j <= N; ++j) colptr[j] = j / 2 + 1;          /* 1-based: the odd columns (0-based) hold one entry each */
    for (int64_t i = 0; i < k; ++i) { rowval[i] = 2 * i + 1; nz[i] = 2.0; }
    for (int64_t j = 0; j < N; ++j) b[j] = j % 2 ? -1.0 : 1.0;

    fd_ctx *ctx;
    CHECK(fd_ctx_create(0, NULL, &ctx));
    void *bd, *yd, *nzd;
    if (hipMalloc(&bd, sizeof(double) * (size_t)N) || hipMalloc(&yd, sizeof(double) * (size_t)N) || hipMalloc(&nzd, sizeof(double) * (size_t)k)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    hipMemcpy(bd, b, sizeof(double) * (size_t)N, 1);
    hipMemcpy(nzd, nz, sizeof(double) * (size_t)k, 1);

    fd_csc_solver *solver;
    CHECK(fd_csc_solver_create(ctx, N, colptr, rowval, 8, 1, FD_HOST, &solver));
    CHECK(fd_csc_solver_set_options(solver, 1e-10, 500));
    /* BiCGStab (the default): breakdown */
    int bflags = -1; int64_t biters = -1; double resid = 0, bnorm = 0;
    CHECK(fd_csc_solve_async(solver, 1.0, 1.0, nzd, bd, yd));
    CHECK(fd_csc_solver_status(solver, &bflags, &biters, &resid, &bnorm));
    hipMemcpy(y, yd, sizeof(double) * (size_t)N, 2);
    const int bnan = isnan(y[0]) && isnan(y[N - 1]);
    printf("csc gmres: bicgstab: status %d iterations %lld\n", bflags, (long long)biters);
    /* GMRES(30) on the same handle */
    int gflags = -1, restart = 0, len = -1; int64_t giters = -1; const void *V = NULL, *H = NULL;
    CHECK(fd_csc_solver_set_method(solver, FD_CSC_METHOD_GMRES, 30));
    CHECK(fd_csc_solve_async(solver, 1.0, 1.0, nzd, bd, yd));
    CHECK(fd_csc_solver_status(solver, &gflags, &giters, &resid, &bnorm));
    CHECK(fd_csc_solver_gmres_basis(solver, &V, &H, &restart, &len));
    hipMemcpy(y, yd, sizeof(double) * (size_t)N, 2);
    double err = 0;
    for (int64_t j = 0; j < N; ++j) err = fmax(err, fabs(y[j] - (j % 2 ? -1.0 : 3.0)));
    printf("csc gmres: gmres(%d): status %d iterations %lld ||r|| / ||b|| = %.3e  max error %.3e\n", restart, gflags, (long long)giters,
           bnorm > 0 ? resid / bnorm : 0.0, err);
    const int ok = bflags == 2 && biters == 0 && bnan && gflags == 0 && giters == 2 && err / 3.0 <= 1e-9 && V != NULL && H != NULL && restart == 30 && len == 2;
    printf("csc gmres: %s\n", ok ? "PASS" : "FAIL");

    CHECK(fd_csc_solver_destroy(solver));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(bd); hipFree(yd); hipFree(nzd);
    free(colptr); free(rowval); free(nz); free(b); free(y);
    return ok ? 0 : 3;
}
