/* The block ILU(0) preconditioner of the sparse consumer from plain C: the 5-point Laplacian on nx x ny points written into CSC storage
 * on the host and uploaded; (I - gamma J) y = b by fd_csc_solve_async with the diagonal and then after
 * fd_csc_solver_set_block_ilu(solver, 256); prints both statuses and the true residual.
 *
 *   gcc -O2 -Iinclude examples/csc_ilu_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
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
    const int64_t nx = 96, ny = 80, N = nx * ny;
    int64_t *colptr = malloc(sizeof(int64_t) * (size_t)(N + 1)), *rowval = malloc(sizeof(int64_t) * (size_t)(5 * N));
    double *nz = malloc(sizeof(double) * (size_t)(5 * N)), *b = malloc(sizeof(double) * (size_t)N);
    int64_t nnz = 0;
    for (int64_t k = 0; k < N; ++k) {                /* column k, 1-based rows ascending */
        const int64_t i = k % nx, j = k / nx;
        colptr[k] = nnz + 1;
        if (j > 0) { rowval[nnz] = k - nx + 1; nz[nnz++] = 1.0; }
        if (i > 0) { rowval[nnz] = k; nz[nnz++] = 1.0; }
        rowval[nnz] = k + 1; nz[nnz++] = -4.0;
        if (i < nx - 1) { rowval[nnz] = k + 2; nz[nnz++] = 1.0; }
        if (j < ny - 1) { rowval[nnz] = k + nx + 1; nz[nnz++] = 1.0; }
    }
    colptr[N] = nnz + 1;
    for (int64_t k = 0; k < N; ++k) b[k] = cos(0.37 * (double)k);

    fd_ctx *ctx;
    CHECK(fd_ctx_create(0, NULL, &ctx));
    void *bd, *yd, *nzd;
    if (hipMalloc(&bd, sizeof(double) * (size_t)N) || hipMalloc(&yd, sizeof(double) * (size_t)N) || hipMalloc(&nzd, sizeof(double) * (size_t)nnz)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    hipMemcpy(bd, b, sizeof(double) * (size_t)N, 1);
    hipMemcpy(nzd, nz, sizeof(double) * (size_t)nnz, 1);

    const double gamma = 10.0;
    fd_csc_solver *solver;
    CHECK(fd_csc_solver_create(ctx, N, colptr, rowval, 8, 1, FD_HOST, &solver));
    CHECK(fd_csc_solver_set_options(solver, 1e-10, 500));
    /* the diagonal alone (the default) */
    int jflags = -1; int64_t jiters = -1; double resid = 0, bnorm = 0;
    CHECK(fd_csc_solve_async(solver, 1.0, -gamma, nzd, bd, yd));
    CHECK(fd_csc_solver_status(solver, &jflags, &jiters, &resid, &bnorm));
    /* ILU(0) inside blocks of 256 rows */
    int flags = -1; int64_t iters = -1;
    CHECK(fd_csc_solver_set_block_ilu(solver, 256));
    CHECK(fd_csc_solve_async(solver, 1.0, -gamma, nzd, bd, yd));
    CHECK(fd_csc_solver_status(solver, &flags, &iters, &resid, &bnorm));
    int64_t nblocks = 0; int bs = 0, max_fwd = -1, max_bwd = -1; const void *lu = NULL, *u = NULL;
    CHECK(fd_csc_solver_ilu_factors(solver, &lu, &u, &nblocks, &bs));
    CHECK(fd_csc_solver_ilu_levels(solver, NULL, NULL, &max_fwd, &max_bwd));

    /* the true residual of (I - gamma J) y = b */
    double *y = malloc(sizeof(double) * (size_t)N), *r = malloc(sizeof(double) * (size_t)N);
    hipMemcpy(y, yd, sizeof(double) * (size_t)N, 2);
    for (int64_t k = 0; k < N; ++k) r[k] = y[k] - b[k];
    for (int64_t k = 0; k < N; ++k)
        for (int64_t q = colptr[k] - 1; q < colptr[k + 1] - 1; ++q) r[rowval[q] - 1] -= gamma * nz[q] * y[k];
    double r2 = 0, b2 = 0;
    for (int64_t k = 0; k < N; ++k) { r2 += r[k] * r[k]; b2 += b[k] * b[k]; }
    const double rel = sqrt(r2 / b2);
    printf("csc ilu: N = %lld nnz = %lld | jacobi: status %d iterations %lld | block ILU(0) (%lld blocks of %d, %d + %d levels): status %d "
           "iterations %lld ||r|| / ||b|| = %.3e  true %.3e\n", (long long)N, (long long)nnz, jflags, (long long)jiters, (long long)nblocks, bs,
           max_fwd + 1, max_bwd + 1, flags, (long long)iters, bnorm > 0 ? resid / bnorm : 0.0, rel);
    const int ok = jflags == 0 && flags == 0 && rel <= 1e-9 && iters < jiters && lu != NULL && u != NULL && nblocks == (N + 255) / 256 && bs == 256;
    printf("csc ilu: %s\n", ok ? "PASS" : "FAIL");

    CHECK(fd_csc_solver_destroy(solver));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(bd); hipFree(yd); hipFree(nzd);
    free(colptr); free(rowval); free(nz); free(b); free(y); free(r);
    return ok ? 0 : 3;
}
