/* The trust-region consumer from plain C: the Hessian (CSC destination) and the gradient of a chain objective that is CONCAVE in every
 * third coordinate, both left on the device, then ONE trust-region step  min g.y + y.H y / 2, ||y|| <= radius  on them by fd_csc_tr_step_async (Steihaug-Toint
 * truncated CG).  H is indefinite at x, so the step follows a direction of negative curvature to the boundary (exit 2); prints the status
 * and the model value q(y) evaluated on the host from the downloaded H and g.
 *
 *   gcc -O2 -Iinclude examples/csc_tr_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
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

/* phi_r = s_r 2 b^2 + b^4 / 12 + 0.1 (a - 2 b + c)^2 with b = x_r, its neighbours a, c and s_r = -1 for r = 0 mod 3, + 1 otherwise */
static const char *SRC =
    "struct ConcaveChain {\n"
    "    long long n;\n"
    "    template <class P> __device__ real_t operator()(long long r, const P &X) const\n"
    "    {\n"
    "        const real_t b = X(r), a0 = X(r > 0 ? r - 1 : r), c0 = X(r + 1 < n ? r + 1 : r);\n"
    "        const real_t a = r > 0 ? a0 : 0.0, c = r + 1 < n ? c0 : 0.0;\n"
    "        const real_t d = (a - 2 * b) + c;\n"
    "        return (b * b * b * b / 12 + (r % 3 == 0 ? -2.0 : 2.0) * b * b) + 0.1 * d * d;\n"
    "    }\n"
    "};\n";

int main(void)
{
    const int64_t n = 2000;
    /* S: row r reads x_{r-1}, x_r, x_{r+1} (0-based) */
    int64_t *scp = malloc(sizeof(int64_t) * (size_t)(n + 1)), *srv = malloc(sizeof(int64_t) * (size_t)(3 * n));
    int64_t k = 0;
    for (int64_t j = 0; j < n; ++j) {
        scp[j] = k;
        for (int64_t r = j - 1; r <= j + 1; ++r) if (r >= 0 && r < n) srv[k++] = r;
    }
    scp[n] = k;
    double *x = malloc(sizeof(double) * (size_t)n);
    for (int64_t j = 0; j < n; ++j) x[j] = 0.5 * sin((double)(j + 1));

    fd_ctx *ctx;
    CHECK(fd_ctx_create(0, NULL, &ctx));
    fd_objective *obj;
    const int64_t prm[1] = {n};
    CHECK(fd_objective_compile(ctx, SRC, "ConcaveChain", prm, sizeof prm, n, n, &obj));
    fd_hess_plan *plan;
    CHECK(fd_hess_plan_create(ctx, n, n, scp, srv, 8, 0, FD_HESS_CSC, 0, &plan));
    int64_t nnz = 0;
    CHECK(fd_hess_plan_info(plan, FD_HESS_INFO_NNZ, &nnz));
    int64_t *colptr = malloc(sizeof(int64_t) * (size_t)(n + 1)), *rowval = malloc(sizeof(int64_t) * (size_t)nnz);
    CHECK(fd_hess_plan_pattern(plan, colptr, rowval));

    void *xd, *Hd, *gd, *yd, *rd;
    if (hipMalloc(&xd, sizeof(double) * (size_t)n) || hipMalloc(&Hd, sizeof(double) * (size_t)nnz) || hipMalloc(&gd, sizeof(double) * (size_t)n) ||
        hipMalloc(&yd, sizeof(double) * (size_t)n) || hipMalloc(&rd, sizeof(double) * (size_t)n)) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    hipMemcpy(xd, x, sizeof(double) * (size_t)n, 1);

    /* Hessian, gradient and the step on one stream: nothing crosses to the host in between */
    const double radius = 50.0;
    fd_csc_tr *tr;
    CHECK(fd_csc_tr_create(ctx, n, colptr, rowval, 8, 0, FD_HOST, &tr));
    CHECK(fd_hessian_async(plan, obj, xd, -1.0, -1.0, Hd));
    CHECK(fd_gradient_async(plan, obj, xd, FD_CENTRAL, -1.0, -1.0, 1.0, gd));
    CHECK(fd_csc_tr_step_async(tr, 0.0, radius, FD_CSC_TR_NORM_IDENTITY, Hd, gd, yd, rd));
    int flags = -1, exit_kind = -1; int64_t iters = -1; double resid = 0, gnorm = 0, ynorm = 0, pred = 0;
    CHECK(fd_csc_tr_status(tr, &flags, &exit_kind, &iters, &resid, &gnorm, &ynorm, &pred));

    /* q(y) from the downloaded values */
    double *H = malloc(sizeof(double) * (size_t)nnz), *g = malloc(sizeof(double) * (size_t)n), *y = malloc(sizeof(double) * (size_t)n);
    hipMemcpy(H, Hd, sizeof(double) * (size_t)nnz, 2);
    hipMemcpy(g, gd, sizeof(double) * (size_t)n, 2);
    hipMemcpy(y, yd, sizeof(double) * (size_t)n, 2);
    long double q = 0, yy = 0;
    for (int64_t j = 0; j < n; ++j) {
        q += (long double)g[j] * y[j];
        yy += (long double)y[j] * y[j];
        for (int64_t s = colptr[j]; s < colptr[j + 1]; ++s) q += 0.5L * (long double)H[s] * y[rowval[s]] * y[j];
    }
    printf("csc tr: N = %lld nnz = %lld status %d exit %d iterations %lld ||y|| = %.15g (radius %g) pred = %.6e  q(y) = %.6e\n", (long long)n,
           (long long)nnz, flags, exit_kind, (long long)iters, ynorm, radius, pred, (double)q);
    const int ok = flags == 0 && exit_kind == 2 && q < 0 && fabs((double)sqrtl(yy) - radius) <= 1e-12 * radius &&
                   fabs(pred + (double)q) <= 1e-9 * fabs((double)q);

    CHECK(fd_csc_tr_destroy(tr));
    CHECK(fd_hess_plan_destroy(plan));
    CHECK(fd_objective_destroy(obj));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(xd); hipFree(Hd); hipFree(gd); hipFree(yd); hipFree(rd);
    free(scp); free(srv); free(x); free(colptr); free(rowval); free(H); free(g); free(y);
    return ok ? 0 : 3;
}
