/* Newton-Krylov's usual pairing from plain C: the MATRIX-FREE operator at the current x, preconditioned by a factorisation of a
 * Jacobian STORED some steps ago.  For the built-in nonlinear tridiagonal family (f_i = x_i-1 - 2 x_i + x_i+1 + x_i^2 x_i+1):
 *   1. a CSC plan writes J(x0) into nzval on the device;
 *   2. a sparse consumer selects block ILU(0) and factors I - gamma J(x0) once (fd_csc_solver_factor_async);
 *   3. the matrix-free consumer borrows that handle (fd_jfnk_solver_set_csc_preconditioner) and solves (I - gamma J(x)) y = b twice,
 *      at x0 and at a moved x1, with the ONE factorisation: it is lagged by design;
 *   4. both iteration counts are printed beside those of the same solves without a preconditioner.
 * The check: both preconditioned solves converge, and neither takes more steps than its unpreconditioned twin.
 *
 *   gcc -O2 -Iinclude examples/jfnk_precond_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
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

static int solve(fd_jfnk_solver *s, double gamma, fd_f_launch f, void *fctx, const void *xd, const void *bd, void *yd, int *flags, int64_t *iters)
{
    double resid = 0.0, bnorm = 0.0;
    CHECK(fd_jfnk_solve_async(s, 1.0, -gamma, f, fctx, xd, NULL, bd, yd));
    CHECK(fd_jfnk_solver_status(s, flags, iters, &resid, &bnorm));
    return 0;
}

int main(void)
{
    const int64_t N = 20000;
    const double gamma = 0.5, rtol = 1e-8;
    const size_t bytes = sizeof(double) * (size_t)N;
    /* the tridiagonal pattern, 1-based, and the cyclic 3-colouring */
    int64_t *colptr = malloc(sizeof(int64_t) * (size_t)(N + 1)), *rowval = malloc(sizeof(int64_t) * (size_t)(3 * N)), *colors = malloc(sizeof(int64_t) * (size_t)N);
    int64_t nnz = 0;
    for (int64_t j = 0; j < N; ++j) {
        colptr[j] = nnz + 1;
        if (j > 0) rowval[nnz++] = j;
        rowval[nnz++] = j + 1;
        if (j + 1 < N) rowval[nnz++] = j + 2;
        colors[j] = j % 3 + 1;
    }
    colptr[N] = nnz + 1;
    double *x0 = malloc(bytes), *x1 = malloc(bytes), *b = malloc(bytes);
    for (int64_t i = 0; i < N; ++i) {
        x0[i] = -0.25 + (double)((i * 7919) % 1000) / 1000.0;
        x1[i] = x0[i] + 0.05 * (double)((i * 104729) % 1000) / 1000.0;
        b[i] = -1.0 + 2.0 * (double)((i * 15485863) % 1000) / 1000.0;
    }
    fd_ctx *ctx;
    CHECK(fd_ctx_create(0, NULL, &ctx));
    fd_f_launch f;
    void *fctx;
    const int64_t prm[1] = {N};
    CHECK(fd_builtin_f_create(ctx, FD_F_TRIDIAG_NL, prm, 1, &f, &fctx));
    void *x0d, *x1d, *bd, *yd, *nzd;
    if (hipMalloc(&x0d, bytes) || hipMalloc(&x1d, bytes) || hipMalloc(&bd, bytes) || hipMalloc(&yd, bytes) || hipMalloc(&nzd, sizeof(double) * (size_t)nnz)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    if (hipMemcpy(x0d, x0, bytes, 1) || hipMemcpy(x1d, x1, bytes, 1) || hipMemcpy(bd, b, bytes, 1)) return 1;

    /* 1. J(x0), stored by a CSC plan */
    fd_plan *plan;
    fd_plan_opts o;
    memset(&o, 0, sizeof o);
    o.fdtype = FD_FORWARD;
    CHECK(fd_plan_create_csc(ctx, N, N, colptr, rowval, 8, 1, colors, 8, &o, &plan));
    void *outs[3] = {nzd, NULL, NULL};
    CHECK(fd_jacobian_async(plan, f, fctx, x0d, NULL, -1.0, -1.0, 1.0, outs));

    /* 2. block ILU(0) of I - gamma J(x0), once */
    fd_csc_solver *pc;
    CHECK(fd_csc_solver_create(ctx, N, colptr, rowval, 8, 1, FD_HOST, &pc));
    CHECK(fd_csc_solver_set_block_ilu(pc, 1024));
    CHECK(fd_csc_solver_factor_async(pc, 1.0, -gamma, nzd));
    int fflags = -1;
    CHECK(fd_csc_solver_factor_status(pc, &fflags));

    /* 3. two solves with the one factorisation, and their twins without it */
    fd_jfnk_solver *s;
    CHECK(fd_jfnk_solver_create(ctx, N, FD_CENTRAL, 30, &s));
    CHECK(fd_jfnk_solver_set_options(s, rtol, 300));
    int flags[4] = {-1, -1, -1, -1};
    int64_t iters[4] = {-1, -1, -1, -1};
    CHECK(solve(s, gamma, f, fctx, x0d, bd, yd, &flags[0], &iters[0]));
    CHECK(solve(s, gamma, f, fctx, x1d, bd, yd, &flags[1], &iters[1]));
    CHECK(fd_jfnk_solver_set_csc_preconditioner(s, pc));
    CHECK(solve(s, gamma, f, fctx, x0d, bd, yd, &flags[2], &iters[2]));
    CHECK(solve(s, gamma, f, fctx, x1d, bd, yd, &flags[3], &iters[3]));

    /* 4. */
    printf("jfnk_precond: factor status %d\n", fflags);
    printf("jfnk_precond: no preconditioner: x0 status %d iterations %lld, x1 status %d iterations %lld\n", flags[0], (long long)iters[0], flags[1],
           (long long)iters[1]);
    printf("jfnk_precond: lagged block ILU : x0 status %d iterations %lld, x1 status %d iterations %lld\n", flags[2], (long long)iters[2], flags[3],
           (long long)iters[3]);
    const int ok = fflags == 0 && flags[2] == 0 && flags[3] == 0 && iters[2] >= 1 && iters[3] >= 1 && (flags[0] != 0 || iters[2] <= iters[0]) &&
                   (flags[1] != 0 || iters[3] <= iters[1]);
    CHECK(fd_jfnk_solver_set_csc_preconditioner(s, NULL));
    CHECK(fd_jfnk_solver_destroy(s));
    CHECK(fd_csc_solver_destroy(pc));
    CHECK(fd_plan_destroy(plan));
    CHECK(fd_builtin_f_destroy(fctx));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(x0d); hipFree(x1d); hipFree(bd); hipFree(yd); hipFree(nzd);
    free(x0); free(x1); free(b); free(colptr); free(rowval); free(colors);
    printf("jfnk_precond: %s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
