/* The pivoted tridiagonal solve from plain C (device pointers through the boundary): W = I - gamma J for a centrally differenced
 * advection term, J = tridiag(c/2h, 0, -c/2h), with gamma c / h = 3 -- W = tridiag(-1.5, 1, 1.5) has no diagonal dominance.  The default
 * elimination refuses it (status bit 0, y = NaN); after fd_tridiag_solver_set_pivoting(solver, 1) the same handle solves it (bit 0 is
 * still reported, bit 2 clear) and the residual ||W y - b||_inf is checked on the host.  Prints both status words.
 *
 *   gcc -O2 -Iinclude examples/tridiag_pivot_client.c -Lfinitediff.jl_amd/lib -lfdjac -L/opt/rocm/lib -lamdhip64 -lm */
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
    const int64_t N = 20011;                       /* three levels: 20011 -> 5004 -> 1252 (the top) */
    const double gamma = 0.5, c_over_2h = 3.0;     /* gamma c / h = 3 */
    const size_t bytes = sizeof(double) * (size_t)N;
    double *dl = malloc(bytes), *d = malloc(bytes), *du = malloc(bytes), *b = malloc(bytes), *y = malloc(bytes);
    for (int64_t i = 0; i < N; ++i) {
        dl[i] = c_over_2h; d[i] = 0.0; du[i] = -c_over_2h;       /* J[i+1, i], J[i, i], J[i, i+1] */
        b[i] = sin(0.01 * (double)i) + (i % 7 == 0 ? 1.0 : 0.0);
    }
    fd_ctx *ctx;
    CHECK(fd_ctx_create(0, NULL, &ctx));
    void *dld, *dd, *dud, *bd, *yd;
    if (hipMalloc(&dld, bytes) || hipMalloc(&dd, bytes) || hipMalloc(&dud, bytes) || hipMalloc(&bd, bytes) || hipMalloc(&yd, bytes)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    hipMemcpy(dld, dl, bytes, 1); hipMemcpy(dd, d, bytes, 1); hipMemcpy(dud, du, bytes, 1); hipMemcpy(bd, b, bytes, 1);
    const void *J[3] = {dld, dd, dud};

    fd_tridiag_solver *solver;
    CHECK(fd_tridiag_solver_create(ctx, N, 0, 0, FD_TRI_DIAGONALS, &solver));
    int off = -1, on = -1;
    CHECK(fd_tridiag_solve_async(solver, 1.0, -gamma, J, bd, yd, NULL));        /* pivoting off: refused */
    CHECK(fd_tridiag_solver_status(solver, &off));
    hipMemcpy(y, yd, bytes, 2);
    const int refused = isnan(y[0]) && isnan(y[N / 2]) && isnan(y[N - 1]);
    printf("tridiag pivot: pivoting off: status %d, y %s\n", off, refused ? "NaN" : "finite");
    CHECK(fd_tridiag_solver_set_pivoting(solver, 1));
    CHECK(fd_tridiag_solve_async(solver, 1.0, -gamma, J, bd, yd, NULL));
    CHECK(fd_tridiag_solver_status(solver, &on));
    hipMemcpy(y, yd, bytes, 2);
    double res = 0, ynorm = 0, bnorm = 0;
    for (int64_t i = 0; i < N; ++i) {
        double r = (1.0 - gamma * d[i]) * y[i] - b[i];
        if (i > 0) r += -gamma * dl[i - 1] * y[i - 1];
        if (i + 1 < N) r += -gamma * du[i] * y[i + 1];
        res = fmax(res, fabs(r));
        ynorm = fmax(ynorm, fabs(y[i]));
        bnorm = fmax(bnorm, fabs(b[i]));
    }
    /* a backward-stable solve: ||W y - b|| <= small multiple of eps ||W|| ||y||, ||W||_inf = 4 */
    const double bound = 64.0 * 2.220446049250313e-16 * (4.0 * ynorm + bnorm);
    printf("tridiag pivot: pivoting on: status %d, residual %.3e (bound %.3e), max |y| %.3e\n", on, res, bound, ynorm);
    const int ok = off == 1 && refused && on == 1 && res <= bound && ynorm > 0 && isfinite(ynorm);
    printf("tridiag pivot: %s\n", ok ? "PASS" : "FAIL");

    CHECK(fd_tridiag_solver_destroy(solver));
    CHECK(fd_ctx_destroy(ctx));
    hipFree(dld); hipFree(dd); hipFree(dud); hipFree(bd); hipFree(yd);
    free(dl); free(d); free(du); free(b); free(y);
    return ok ? 0 : 3;
}
