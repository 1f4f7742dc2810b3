/* The block-Jacobi preconditioner of the sparse consumer from plain C: the Jacobian of a reaction-diffusion residual on nx x ny cells
 * with m = 4 strongly and non-symmetrically coupled species per cell (the species the fastest index), written into CSC storage on the
 * host and uploaded; (I - gamma J) y = b by fd_csc_solve_async after fd_csc_solver_set_preconditioner(solver,
 * FD_CSC_PRECOND_BLOCK_JACOBI, 4); prints the status of that solve, of the diagonal-preconditioned one beside it, and the true residual.
 *
 *   gcc -O2 -Iinclude examples/csc_precond_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
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

enum { M_SPECIES = 4 };

/* dJ_(cell, t) / dx_(cell, s): the reaction's coupling inside a cell, stiff (k) and not symmetric */
static double coupling(int t, int s, int64_t cell)
{
    const double k = 200.0, d = (double)(t - s);
    const double sym = 1.0 / (1.0 + d * d), skew = t == s ? 0.0 : (s > t ? 0.6 : -0.6);
    return -k * (sym + skew) * (1.0 + 0.1 * sin((double)cell));
}

int main(void)
{
    const int64_t nx = 48, ny = 40, m = M_SPECIES, ncell = nx * ny, N = ncell * m;
    int64_t *colptr = malloc(sizeof(int64_t) * (size_t)(N + 1)), *rowval = malloc(sizeof(int64_t) * (size_t)((m + 4) * N));
    double *nz = malloc(sizeof(double) * (size_t)((m + 4) * N)), *b = malloc(sizeof(double) * (size_t)N);
    int64_t nnz = 0;
    for (int64_t cell = 0; cell < ncell; ++cell) {
        const int64_t i = cell % nx, j = cell / nx;
        for (int64_t s = 0; s < m; ++s) {            /* column (cell, s), 1-based rows ascending */
            const double c = 0.5 + (double)s / (double)(m - 1);
            colptr[cell * m + s] = nnz + 1;
            if (j > 0) { rowval[nnz] = (cell - nx) * m + s + 1; nz[nnz++] = c; }
            if (i > 0) { rowval[nnz] = (cell - 1) * m + s + 1; nz[nnz++] = c; }
            for (int64_t t = 0; t < m; ++t) { rowval[nnz] = cell * m + t + 1; nz[nnz++] = coupling((int)t, (int)s, cell) + (t == s ? -4.0 * c : 0.0); }
            if (i < nx - 1) { rowval[nnz] = (cell + 1) * m + s + 1; nz[nnz++] = c; }
            if (j < ny - 1) { rowval[nnz] = (cell + nx) * m + s + 1; nz[nnz++] = c; }
        }
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

    const double gamma = 0.1;
    fd_csc_solver *solver;
    CHECK(fd_csc_solver_create(ctx, N, colptr, rowval, 8, 1, FD_HOST, &solver));
    CHECK(fd_csc_solver_set_options(solver, 1e-10, 500));
    /* the diagonal alone, for comparison (the default; said explicitly) */
    int jflags = -1; int64_t jiters = -1; double resid = 0, bnorm = 0;
    CHECK(fd_csc_solver_set_preconditioner(solver, FD_CSC_PRECOND_JACOBI, 0));
    CHECK(fd_csc_solve_async(solver, 1.0, -gamma, nzd, bd, yd));
    CHECK(fd_csc_solver_status(solver, &jflags, &jiters, &resid, &bnorm));
    /* one block per cell */
    int flags = -1; int64_t iters = -1;
    CHECK(fd_csc_solver_set_preconditioner(solver, FD_CSC_PRECOND_BLOCK_JACOBI, (int)m));
    CHECK(fd_csc_solve_async(solver, 1.0, -gamma, nzd, bd, yd));
    CHECK(fd_csc_solver_status(solver, &flags, &iters, &resid, &bnorm));
    int64_t nblocks = 0; int bs = 0; const void *inv = NULL;
    CHECK(fd_csc_solver_block_inverses(solver, &inv, &nblocks, &bs));

    /* the true residual of (I - gamma J) y = b */
    double *y = malloc(sizeof(double) * (size_t)N), *r = malloc(sizeof(double) * (size_t)N);
    hipMemcpy(y, yd, sizeof(double) * (size_t)N, 2);
    for (int64_t k = 0; k < N; ++k) r[k] = y[k] - b[k];
    for (int64_t k = 0; k < N; ++k)
        for (int64_t q = colptr[k] - 1; q < colptr[k + 1] - 1; ++q) r[rowval[q] - 1] -= gamma * nz[q] * y[k];
    double r2 = 0, b2 = 0;
    for (int64_t k = 0; k < N; ++k) { r2 += r[k] * r[k]; b2 += b[k] * b[k]; }
    const double rel = sqrt(r2 / b2);
    printf("csc precond: N = %lld nnz = %lld | jacobi: status %d iterations %lld | block jacobi (%lld blocks of %d): status %d iterations %lld "
           "||r|| / ||b|| = %.3e  true %.3e\n", (long long)N, (long long)nnz, jflags, (long long)jiters, (long long)nblocks, bs, flags, (long long)iters,
           bnorm > 0 ? resid / bnorm : 0.0, rel);
    const int ok = flags == 0 && rel <= 1e-9 && inv != NULL && nblocks == ncell && bs == (int)m;      /* (the diagonal's solve is printed, not judged) */
    printf("csc precond: %s\n", ok ? "PASS" : "FAIL");

    CHECK(fd_csc_solver_destroy(solver));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(bd); hipFree(yd); hipFree(nzd);
    free(colptr); free(rowval); free(nz); free(b); free(y); free(r);
    return ok ? 0 : 3;
}
