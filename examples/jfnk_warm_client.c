/* The matrix-free consumer's warm start from plain C: the system of examples/jfnk_client.c ((I - gamma J(x)) y = b on the built-in
 * tridiagonal family, b = (I - gamma J) 1, so y = 1), solved with max_iterations = 3 under the keep policy and then CONTINUED IN PLACE
 * -- fd_jfnk_solve_from_async with y0 == y -- until the status says converged.  Device pointers go through the boundary.  Prints the
 * calls, the iterations of every call, the last estimate and ||y - 1||_2; the check is jfnk_client.c's.
 *
 *   gcc -O2 -Iinclude examples/jfnk_warm_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
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
    const int64_t N = 20001;
    const double gamma = 0.3, rtol = 1e-6;
    const int cap = 3, max_calls = 50;
    const size_t bytes = sizeof(double) * (size_t)N;
    double *x = malloc(bytes), *b = malloc(bytes), *y = malloc(bytes);
    double bn2 = 0.0;
    for (int64_t i = 0; i < N; ++i) {
        x[i] = 0.25 + 0.5 * (double)(i % 7) / 7.0;
        const double ji = -2.0 + (i > 0 ? 1.0 : 0.0) + (i + 1 < N ? 1.0 : 0.0);      /* row i of J times the vector of ones */
        b[i] = 1.0 - gamma * ji;
        bn2 += b[i] * b[i];
    }
    fd_ctx *ctx;
    CHECK(fd_ctx_create(0, NULL, &ctx));
    fd_f_launch f;
    void *fctx;
    const int64_t prm[1] = {N};
    CHECK(fd_builtin_f_create(ctx, FD_F_TRIDIAG, prm, 1, &f, &fctx));
    fd_f_launch_lazy_jvp lazy;
    int caps = 0;
    CHECK(fd_builtin_f_lazy_jvp(fctx, &lazy));
    CHECK(fd_builtin_f_lazy_jvp_caps(fctx, &caps));
    void *xd, *bd, *yd;
    if (hipMalloc(&xd, bytes) || hipMalloc(&bd, bytes) || hipMalloc(&yd, bytes)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    if (hipMemcpy(xd, x, bytes, 1) || hipMemcpy(bd, b, bytes, 1)) return 1;

    fd_jfnk_solver *s;
    CHECK(fd_jfnk_solver_create(ctx, N, FD_FORWARD, 30, &s));
    CHECK(fd_jfnk_solver_set_options(s, rtol, cap));
    CHECK(fd_jfnk_solver_set_policy(s, 1));          /* a solve that runs out of iterations leaves its iterate in y */
    CHECK(fd_jfnk_solver_set_lazy_f(s, lazy, caps));
    int flags = -1, calls = 0;
    int64_t iters = -1, total = 0;
    double resid = 0.0, bnorm = 0.0;
    do {
        if (calls == 0) CHECK(fd_jfnk_solve_async(s, 1.0, -gamma, f, fctx, xd, NULL, bd, yd));
        else CHECK(fd_jfnk_solve_from_async(s, 1.0, -gamma, f, fctx, xd, NULL, bd, yd, yd));          /* y0 is y */
        CHECK(fd_jfnk_solver_status(s, &flags, &iters, &resid, &bnorm));
        ++calls;
        total += iters;
        printf("jfnk warm: call %d: status %d iterations %lld estimate %.17g\n", calls, flags, (long long)iters, resid);
    } while (flags == 1 && calls < max_calls);
    if (hipMemcpy(y, yd, bytes, 2)) return 1;
    double err2 = 0.0;
    for (int64_t i = 0; i < N; ++i) err2 += (y[i] - 1.0) * (y[i] - 1.0);
    printf("jfnk warm: %d calls, %lld iterations, ||y - 1||_2 = %.3e (allowed %.3e)\n", calls, (long long)total, sqrt(err2), 2.0 * rtol * sqrt(bn2));
    const int ok = flags == 0 && calls >= 2 && sqrt(err2) <= 2.0 * rtol * sqrt(bn2);
    CHECK(fd_jfnk_solver_destroy(s));
    CHECK(fd_builtin_f_destroy(fctx));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(xd); hipFree(bd); hipFree(yd);
    free(x); free(b); free(y);
    printf("jfnk warm: %s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
