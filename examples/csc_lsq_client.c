/* The least-squares consumer from plain C: the Jacobian of a built-in rectangular residual (n rows, 2n unknowns) through a CSC plan,
 * left on the device, then ONE Levenberg step  y = argmin ||J y - b||^2 + mu ||y||^2  on the stored nzval by fd_csc_lsq_solve_async;
 * prints the status and the true gradient J^T (b - J y) - mu y.
 *
 *   gcc -O2 -Iinclude examples/csc_lsq_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
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
    const int64_t n = 3000, M = n, N = 2 * n, nnz = N;
    /* f_i = (x_i - 3)^2 + x_i x_{n+i} + (x_{n+i} + 4)^2 - 3: column j holds row j mod n (1-based, as Julia stores it); two colours */
    int64_t *colptr = malloc(sizeof(int64_t) * (size_t)(N + 1)), *rowval = malloc(sizeof(int64_t) * (size_t)nnz);
    int64_t *colors = malloc(sizeof(int64_t) * (size_t)N);
    for (int64_t j = 0; j < N; ++j) { colptr[j] = j + 1; rowval[j] = j % n + 1; colors[j] = j < n ? 1 : 2; }
    colptr[N] = nnz + 1;
    double *x = malloc(sizeof(double) * (size_t)N), *b = malloc(sizeof(double) * (size_t)M);
    for (int64_t k = 0; k < N; ++k) x[k] = 1.5 + 0.5 * sin((double)(k + 1));
    for (int64_t k = 0; k < M; ++k) b[k] = cos(0.37 * (double)k);

    fd_ctx *ctx;
    CHECK(fd_ctx_create(0, NULL, &ctx));
    void *xd, *bd, *yd, *rd, *nzd;
    if (hipMalloc(&xd, sizeof(double) * (size_t)N) || hipMalloc(&bd, sizeof(double) * (size_t)M) || hipMalloc(&yd, sizeof(double) * (size_t)N) ||
        hipMalloc(&rd, sizeof(double) * (size_t)M) || hipMalloc(&nzd, sizeof(double) * (size_t)nnz)) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    hipMemcpy(xd, x, sizeof(double) * (size_t)N, 1);
    hipMemcpy(bd, b, sizeof(double) * (size_t)M, 1);

    /* the Jacobian: forward differences, stored as SparseMatrixCSC nzval on the device */
    fd_f_launch f; void *fctx; fd_plan *plan;
    const int64_t prm[1] = {n};
    CHECK(fd_builtin_f_create(ctx, FD_F_NONSQUARE, prm, 1, &f, &fctx));
    fd_plan_opts o; memset(&o, 0, sizeof o); o.fdtype = FD_FORWARD;
    CHECK(fd_plan_create_csc(ctx, M, N, colptr, rowval, 8, 1, colors, 8, &o, &plan));
    void *outs[3] = {nzd, NULL, NULL};
    CHECK(fd_jacobian_async(plan, f, fctx, xd, NULL, -1.0, -1.0, 1.0, outs));

    /* the consumer, on the same stream: no synchronisation in between.  M < N: J^T J is singular, Levenberg's mu I makes the step unique */
    const double mu = 0.5;
    fd_csc_lsq *lsq;
    CHECK(fd_csc_lsq_create(ctx, M, N, colptr, rowval, 8, 1, FD_HOST, &lsq));
    CHECK(fd_csc_lsq_set_options(lsq, 1e-12, 100));
    CHECK(fd_csc_lsq_solve_async(lsq, mu, FD_CSC_LSQ_DAMP_IDENTITY, nzd, bd, yd, rd));
    int flags = -1; int64_t iters = -1; double grad = 0, grad0 = 0;
    CHECK(fd_csc_lsq_status(lsq, &flags, &iters, &grad, &grad0));

    /* the true gradient from the downloaded values */
    double *nz = malloc(sizeof(double) * (size_t)nnz), *y = malloc(sizeof(double) * (size_t)N), *r = malloc(sizeof(double) * (size_t)M);
    hipMemcpy(nz, nzd, sizeof(double) * (size_t)nnz, 2);
    hipMemcpy(y, yd, sizeof(double) * (size_t)N, 2);
    for (int64_t k = 0; k < M; ++k) r[k] = b[k];
    for (int64_t j = 0; j < N; ++j) r[rowval[j] - 1] -= nz[j] * y[j];
    double worst = 0;
    for (int64_t j = 0; j < N; ++j) {
        const double s = nz[j] * r[rowval[j] - 1] - mu * y[j];
        if (!(fabs(s) <= worst)) worst = fabs(s);
    }
    printf("csc lsq: M = %lld N = %lld nnz = %lld status %d iterations %lld ||grad|| / ||grad0|| = %.3e  max|J'(b - J y) - mu y| = %.3e\n", (long long)M,
           (long long)N, (long long)nnz, flags, (long long)iters, grad0 > 0 ? grad / grad0 : 0.0, worst);
    const int ok = flags == 0 && worst <= 1e-9;

    CHECK(fd_csc_lsq_destroy(lsq));
    CHECK(fd_plan_destroy(plan));
    CHECK(fd_builtin_f_destroy(fctx));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(xd); hipFree(bd); hipFree(yd); hipFree(rd); hipFree(nzd);
    free(colptr); free(rowval); free(colors); free(x); free(b); free(nz); free(y); free(r);
    return ok ? 0 : 3;
}
