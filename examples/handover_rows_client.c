/*
 * The row-wise hand-over decompression through the C ABI (FD_PLAN_HANDOVER_ROWS): an OPAQUE f! -- a plain fd_f_launch the plan knows
 * nothing about (here a user's function that forwards to the library's residual for any pattern, FD_F_SPARSE) -- on a small random
 * band, once on a plan with FD_PLAN_STORE_CSC | FD_PLAN_STORE_CSC_ROWS | FD_PLAN_HANDOVER_ROWS and once on a plan without flags.
 * Checks: the flagged plan reports FD_INFO_HANDOVER_ROWS = 1, the other 0; the two nzval are the same bytes (memcmp), forward and
 * central; the flag without FD_PLAN_STORE_CSC_ROWS is FD_ERR_ARG.  Exits non-zero on any difference.
 *
 *   gcc -O2 -Iinclude examples/handover_rows_client.c -o handover_rows_client -Lfinitediff.jl_amd/lib -lfdjac -lm
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fdjac.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s:%d %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, fd_last_error()); return rc_ == FD_ERR_NODEVICE ? 7 : 1; } } while (0)

/* the user's f!: opaque to the plan (no lazy launcher is installed) */
typedef struct { fd_f_launch inner; void *inner_ctx; int64_t calls; } user_f;
static int user_launch(void *fctx, void *fx, const void *x, int64_t nbatch, int64_t x_stride, int64_t fx_stride, int64_t row_begin, int64_t row_end,
                       int is_complex, void *stream)
{
    user_f *u = (user_f *)fctx;
    u->calls += nbatch;
    return u->inner(u->inner_ctx, fx, x, nbatch, x_stride, fx_stride, row_begin, row_end, is_complex, stream);
}

static uint64_t lcg(uint64_t *s) { *s = *s * 6364136223846793005ull + 1442695040888963407ull; return *s >> 33; }

int main(int argc, char **argv)
{
    const int64_t N = argc > 1 ? atoll(argv[1]) : 3001, half = 60, per = 5;
    fd_ctx *ctx = NULL;
    CHECK(fd_ctx_create(0, NULL, &ctx));
    /* the CSC pattern (1-based Int64): `per` distinct rows within +-half of every column, ascending */
    int64_t *colptr = malloc(sizeof(int64_t) * (size_t)(N + 1)), *rowval = malloc(sizeof(int64_t) * (size_t)(per * N)), *colors = malloc(sizeof(int64_t) * (size_t)N);
    uint64_t seed = 12345;
    int64_t p = 0;
    for (int64_t j = 0; j < N; ++j) {
        int64_t rows[8];
        int n = 0;
        colptr[j] = p + 1;
        while (n < per) {
            int64_t r = j - half + (int64_t)(lcg(&seed) % (uint64_t)(2 * half + 1));
            r = r < 0 ? 0 : r >= N ? N - 1 : r;
            int dup = 0;
            for (int k = 0; k < n; ++k) dup |= rows[k] == r;
            if (dup) { if (N < per) break; continue; }
            int k = n++;
            while (k > 0 && rows[k - 1] > r) { rows[k] = rows[k - 1]; --k; }
            rows[k] = r;
        }
        for (int k = 0; k < n; ++k) rowval[p++] = rows[k] + 1;
    }
    colptr[N] = p + 1;
    const int64_t nnz = p;
    int64_t C = 0;
    CHECK(fd_color_columns_greedy(N, N, colptr, rowval, 8, 1, colors, &C));
    double *x = malloc(sizeof(double) * (size_t)N), *a = malloc(sizeof(double) * (size_t)nnz), *b = malloc(sizeof(double) * (size_t)nnz);
    for (int64_t k = 0; k < N; ++k) x[k] = 0.5 + 0.25 * sin((double)(k + 1));
    user_f u = {NULL, NULL, 0};
    CHECK(fd_builtin_f_create_sparse(ctx, N, N, colptr, rowval, 8, 1, &u.inner, &u.inner_ctx));
    int bad = 0;
    {   /* the flag alone is an argument error */
        fd_plan_opts o; memset(&o, 0, sizeof o); o.fdtype = FD_FORWARD; o.flags = FD_PLAN_STORE_CSC | FD_PLAN_HANDOVER_ROWS;
        fd_plan *pe = NULL;
        const int rc = fd_plan_create_csc(ctx, N, N, colptr, rowval, 8, 1, colors, 8, &o, &pe);
        printf("handover_rows: the flag without FD_PLAN_STORE_CSC_ROWS -> %d (%s)\n", rc, rc ? fd_last_error() : "accepted");
        bad |= rc != FD_ERR_ARG;
        if (rc == 0) CHECK(fd_plan_destroy(pe));
    }
    for (int fdtype = FD_FORWARD; fdtype <= FD_CENTRAL; ++fdtype) {
        fd_plan_opts o; memset(&o, 0, sizeof o); o.fdtype = fdtype; o.flags = FD_PLAN_STORE_CSC | FD_PLAN_STORE_CSC_ROWS | FD_PLAN_HANDOVER_ROWS;
        fd_plan *pr = NULL, *pl = NULL;
        CHECK(fd_plan_create_csc(ctx, N, N, colptr, rowval, 8, 1, colors, 8, &o, &pr));
        o.flags = 0;
        CHECK(fd_plan_create_csc(ctx, N, N, colptr, rowval, 8, 1, colors, 8, &o, &pl));
        int64_t rows_on = -1, rows_off = -1;
        CHECK(fd_plan_info(pr, FD_INFO_HANDOVER_ROWS, &rows_on));
        CHECK(fd_plan_info(pl, FD_INFO_HANDOVER_ROWS, &rows_off));
        for (int64_t k = 0; k < nnz; ++k) a[k] = b[k] = -777.0 - (double)k;      /* one sentinel pattern: an untouched slot compares too */
        void *outs1[3] = {a, NULL, NULL}, *outs2[3] = {b, NULL, NULL};
        const int64_t n0 = u.calls;
        CHECK(fd_jacobian(pr, user_launch, &u, x, FD_HOST, NULL, FD_HOST, -1.0, -1.0, 1.0, outs1, FD_HOST));
        const int64_t n1 = u.calls;
        CHECK(fd_jacobian(pl, user_launch, &u, x, FD_HOST, NULL, FD_HOST, -1.0, -1.0, 1.0, outs2, FD_HOST));
        const int64_t n2 = u.calls;
        const int same = memcmp(a, b, sizeof(double) * (size_t)nnz) == 0;
        int64_t written = 0;
        for (int64_t k = 0; k < nnz; ++k) written += a[k] != -777.0 - (double)k;
        const int ok = rows_on == 1 && rows_off == 0 && same && written == nnz && n1 - n0 == n2 - n1;
        printf("handover_rows %s: N %lld, %lld entries, %lld colours, FD_INFO_HANDOVER_ROWS %lld / %lld, %lld slots written, same bytes as the plan "
               "without the flag %s, f! evaluations %lld / %lld  %s\n", fdtype == FD_FORWARD ? "forward" : "central", (long long)N, (long long)nnz,
               (long long)C, (long long)rows_on, (long long)rows_off, (long long)written, same ? "yes" : "NO", (long long)(n1 - n0), (long long)(n2 - n1),
               ok ? "ok" : "FAILED");
        bad |= !ok;
        CHECK(fd_plan_destroy(pr)); CHECK(fd_plan_destroy(pl));
    }
    CHECK(fd_builtin_f_destroy(u.inner_ctx));
    free(a); free(b); free(x); free(colptr); free(rowval); free(colors);
    CHECK(fd_ctx_destroy(ctx));
    printf("%s\n", bad ? "handover_rows_client FAILED" : "handover_rows_client ok");
    return bad ? 3 : 0;
}
