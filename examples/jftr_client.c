/* The matrix-free trust-region consumer from plain C: the Steihaug-Toint step of  min g.y + 1/2 y.B y,  ||y||_2 <= radius,  with
 * B = 1/2 I - J(x) and J(x) v the finite-difference JVP of the built-in tridiagonal family (f_i = x_i-1 - 2 x_i + x_i+1, the gradient of a
 * concave quadratic: J = tridiag(1, -2, 1) whatever x is, so B is positive definite with eigenvalues in [0.5, 4.5]) -- no pattern, no
 * colouring, no stored Hessian.  Device pointers go through the boundary; the family's lazy JVP launcher writes the finished quotient.
 * g = -B 1, so the unconstrained minimiser is y = 1.
 * The checks: without a boundary, ||y - 1||_2 <= ||g + B y||_2 / 0.5, which the step leaves at about 2 rtol ||g||_2; twice that is
 * allowed.  With radius = ||1||_2 / 2 the step ends on the boundary: exit 1, ||y||_2 = radius to 1e-12, pred > 0.
 *
 *   gcc -O2 -Iinclude examples/jftr_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
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
    const double lambda = 0.5, beta = -1.0, rtol = 1e-6;
    const size_t bytes = sizeof(double) * (size_t)N;
    double *x = malloc(bytes), *g = malloc(bytes), *y = malloc(bytes);
    double gn2 = 0.0;
    for (int64_t i = 0; i < N; ++i) {
        x[i] = 0.25 + 0.5 * (double)(i % 7) / 7.0;
        const double ji = -2.0 + (i > 0 ? 1.0 : 0.0) + (i + 1 < N ? 1.0 : 0.0);      /* row i of J times the vector of ones */
        g[i] = -(lambda + beta * ji);
        gn2 += g[i] * g[i];
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
    void *xd, *gd, *yd, *rd;
    if (hipMalloc(&xd, bytes) || hipMalloc(&gd, bytes) || hipMalloc(&yd, bytes) || hipMalloc(&rd, bytes)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    if (hipMemcpy(xd, x, bytes, 1) || hipMemcpy(gd, g, bytes, 1)) return 1;

    fd_jftr *s;
    CHECK(fd_jftr_create(ctx, N, FD_FORWARD, &s));
    CHECK(fd_jftr_set_options(s, rtol, 200));
    CHECK(fd_jftr_set_lazy_f(s, lazy, caps));
    int flags = -1, exit_kind = -1;
    int64_t iters = -1, apps = -1, base = -1;
    double resid = 0.0, gnorm = 0.0, snorm = 0.0, pred = 0.0;

    CHECK(fd_jftr_step_async(s, lambda, beta, INFINITY, f, fctx, xd, NULL, gd, yd, rd));
    CHECK(fd_jftr_status(s, &flags, &exit_kind, &iters, &resid, &gnorm, &snorm, &pred));
    CHECK(fd_jftr_counts(s, &apps, &base));
    if (hipMemcpy(y, yd, bytes, 2)) return 1;
    double err2 = 0.0;
    for (int64_t i = 0; i < N; ++i) err2 += (y[i] - 1.0) * (y[i] - 1.0);
    printf("jftr: no boundary: status %d exit %d iterations %lld ||r|| %.3e ||g|| %.6e ||y|| %.6e pred %.6e applications %lld base evaluations %lld\n",
           flags, exit_kind, (long long)iters, resid, gnorm, snorm, pred, (long long)apps, (long long)base);
    printf("jftr: ||y - 1||_2 = %.3e (allowed %.3e)\n", sqrt(err2), 4.0 * rtol * sqrt(gn2));
    int ok = flags == 0 && exit_kind == 0 && iters >= 1 && base == 1 && apps == iters && sqrt(err2) <= 4.0 * rtol * sqrt(gn2) &&
             fabs(gnorm - sqrt(gn2)) <= 1e-12 * sqrt(gn2) && pred > 0.0;

    const double radius = 0.5 * sqrt((double)N);
    CHECK(fd_jftr_step_async(s, lambda, beta, radius, f, fctx, xd, NULL, gd, yd, NULL));
    CHECK(fd_jftr_status(s, &flags, &exit_kind, &iters, &resid, &gnorm, &snorm, &pred));
    printf("jftr: radius %.6e: status %d exit %d iterations %lld ||y|| %.17g pred %.6e\n", radius, flags, exit_kind, (long long)iters, snorm, pred);
    ok = ok && flags == 0 && exit_kind == 1 && iters >= 1 && fabs(snorm - radius) <= 1e-12 * radius && pred > 0.0;

    CHECK(fd_jftr_destroy(s));
    CHECK(fd_builtin_f_destroy(fctx));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(xd); hipFree(gd); hipFree(yd); hipFree(rd);
    free(x); free(g); free(y);
    printf("jftr: %s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
