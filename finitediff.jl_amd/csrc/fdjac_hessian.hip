// Hessian and gradient of a PARTIALLY SEPARABLE objective f(x) = sum_r phi_r(x) (include/fdjac.h, fd_objective_compile / fd_hessian /
// fd_gradient): finite_difference_hessian! (src/hessians.jl:202-292) and finite_difference_gradient! (src/gradients.jl:407-446).
//
// The reference makes O(n^2) calls to a scalar f of O(n) cost each.  With the rows' support pattern S (row r of column j stored <=> phi_r
// reads x_j) every Hessian entry H_ij is a short sum over rows(i) & rows(j) and every gradient entry a sum over rows(j): O(nnz) work in
// one launch after the rows pass, no colouring, no atomics.  The kernels are templates of include/fdjac_device.h (fd_obj_rows,
// fd_hess_entries, fd_grad_cols), instantiated for the caller's functor by the library's runtime compiler (fdjac_rtc.hip: the one
// fd_f_compile_rows uses -- embedded header, -ffp-contract=off, gfx950); this file names the kernels and keeps the compiled objectives,
// cached by content.  The plan builds P = pattern(S^T S) and the rows of every upper entry on the host, on the first call that needs
// them.  Float64 only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>

#include "fdjac_internal.h"

namespace fdjac {

// one compiled objective: its three kernels
struct ObjModule {
    hipModule_t mod = nullptr;
    hipFunction_t rows = nullptr, hess = nullptr, grad[2] = {nullptr, nullptr};      // grad: [forward / central]
    unsigned sizeof_f = 0;
    int refs = 0;
    std::string key;
    ~ObjModule() { if (mod) (void)hipModuleUnload(mod); }
};
static ModuleCache<ObjModule> g_obj_modules;

static const char kObjTail[] = R"FDOBJ(
typedef FDOBJ_FUNCTOR fdobj_F;
extern "C" __device__ __attribute__((used)) const unsigned fdobj_sizeof_f = sizeof(fdobj_F);
)FDOBJ";

static int require_device()
{
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return FD_ERR_NODEVICE;
    }
    return FD_OK;
}

}  // namespace fdjac

struct fd_objective {
    fd_ctx *ctx = nullptr;
    fdjac::ObjModule *m = nullptr;
    std::vector<unsigned char> params;      // the functor object, byte for byte
    int64_t M = 0, N = 0;
    int64_t launches = 0;
};

struct fd_hess_plan {
    fd_ctx *ctx = nullptr;
    int64_t M = 0, N = 0;
    int dest = 0;
    int64_t band = 0;
    std::vector<int64_t> s_colptr;          // S, 0-based, rows ascending and unique per column
    std::vector<int32_t> s_rowval;
    int64_t bw = 0;                         // P's half-bandwidth: max over rows of (last column - first column)
    long long *d_scolptr = nullptr;         // S on the device (the gradient pass)
    int *d_srowval = nullptr;
    double *d_fx = nullptr;                 // [M] phi_r(x): the rows pass
    // P and the entry lists, built on first use
    bool built = false;
    std::vector<int64_t> p_colptr;
    std::vector<int32_t> p_rowval;
    int64_t nent = 0, ndiag = 0, list_len = 0;
    bool band_full = false;                 // BANDED: P fills every in-matrix slot of the band (only the corner columns need zeros)
    int *d_ent_i = nullptr, *d_ent_j = nullptr, *d_rows = nullptr;
    long long *d_lo = nullptr, *d_dst = nullptr;
    // staging of host x / outputs (fd_hessian, fd_gradient)
    double *d_xstage = nullptr, *d_outstage = nullptr;
    int64_t outstage_n = 0;
};

namespace fdjac {

static int64_t hess_out_len(const fd_hess_plan *p)
{
    if (p->dest == FD_HESS_CSC) return (int64_t)p->p_rowval.size();
    if (p->dest == FD_HESS_BANDED) return (2 * p->band + 1) * p->N;
    return p->N * p->N;
}

template <typename X> static int upload(X **d, const std::vector<X> &h)
{
    if (h.empty()) return FD_OK;
    FD_HIP_CHECK(hipMalloc((void **)d, h.size() * sizeof(X)));
    FD_HIP_CHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(X), hipMemcpyHostToDevice));
    return FD_OK;
}

// P = pattern(S^T S) by columns, and the upper entries (diagonals first, then i < j; each by ascending j, then i) with the ascending
// rows of rows(i) & rows(j) and -- for the CSC destination -- the slots of (i, j) and (j, i) in P's nzval
static int build_pattern(fd_hess_plan *p)
{
    if (p->built) return FD_OK;
    const int64_t M = p->M, N = p->N;
    const std::vector<int64_t> &cp = p->s_colptr;
    const std::vector<int32_t> &rv = p->s_rowval;
    // S by rows (columns ascending)
    std::vector<int64_t> rp(M + 1, 0);
    for (int32_t r : rv) rp[r + 1] += 1;
    for (int64_t r = 0; r < M; ++r) rp[r + 1] += rp[r];
    std::vector<int32_t> rc(rv.size());
    {
        std::vector<int64_t> at(rp.begin(), rp.end() - 1);
        for (int64_t j = 0; j < N; ++j)
            for (int64_t q = cp[j]; q < cp[j + 1]; ++q) rc[at[rv[q]]++] = (int32_t)j;
    }
    // P column j = the union of the columns of the rows of column j
    std::vector<int64_t> pcp(N + 1, 0);
    std::vector<int32_t> prv;
    std::vector<int64_t> mark(N, -1);
    std::vector<int32_t> tmp;
    for (int64_t j = 0; j < N; ++j) {
        tmp.clear();
        for (int64_t q = cp[j]; q < cp[j + 1]; ++q)
            for (int64_t t = rp[rv[q]]; t < rp[rv[q] + 1]; ++t)
                if (mark[rc[t]] != j) { mark[rc[t]] = j; tmp.push_back(rc[t]); }
        std::sort(tmp.begin(), tmp.end());
        prv.insert(prv.end(), tmp.begin(), tmp.end());
        pcp[j + 1] = (int64_t)prv.size();
    }
    // the upper entries and their row lists
    std::vector<int32_t> ei, ej, rows;
    std::vector<int64_t> lo(1, 0), dst;
    const bool csc = p->dest == FD_HESS_CSC;
    auto slot = [&](int64_t col, int64_t row) {
        return pcp[col] + (int64_t)(std::lower_bound(prv.begin() + pcp[col], prv.begin() + pcp[col + 1], (int32_t)row) - (prv.begin() + pcp[col]));
    };
    for (int64_t j = 0; j < N; ++j) {
        if (cp[j] == cp[j + 1]) continue;
        ei.push_back((int32_t)j);
        ej.push_back((int32_t)j);
        rows.insert(rows.end(), rv.begin() + cp[j], rv.begin() + cp[j + 1]);
        lo.push_back((int64_t)rows.size());
        if (csc) { const int64_t s = slot(j, j); dst.push_back(s); dst.push_back(s); }
    }
    const int64_t ndiag = (int64_t)ei.size();
    for (int64_t j = 0; j < N; ++j)
        for (int64_t k = pcp[j]; k < pcp[j + 1] && prv[k] < j; ++k) {
            const int64_t i = prv[k];
            int64_t a = cp[i], b = cp[j];
            while (a < cp[i + 1] && b < cp[j + 1]) {
                if (rv[a] < rv[b]) ++a;
                else if (rv[b] < rv[a]) ++b;
                else { rows.push_back(rv[a]); ++a; ++b; }
            }
            ei.push_back((int32_t)i);
            ej.push_back((int32_t)j);
            lo.push_back((int64_t)rows.size());
            if (csc) { dst.push_back(k); dst.push_back(slot(i, j)); }
        }
    p->nent = (int64_t)ei.size();
    p->ndiag = ndiag;
    p->list_len = (int64_t)rows.size();
    if (p->dest == FD_HESS_BANDED) {
        int64_t inband = 0;
        for (int64_t j = 0; j < N; ++j) inband += std::min<int64_t>(N - 1, j + p->band) - std::max<int64_t>(0, j - p->band) + 1;
        p->band_full = inband == (int64_t)prv.size();
    }
    int rc2 = upload(&p->d_ent_i, ei);
    if (rc2 == FD_OK) rc2 = upload(&p->d_ent_j, ej);
    if (rc2 == FD_OK) rc2 = upload(&p->d_rows, rows);
    if (rc2 == FD_OK) rc2 = upload((int64_t **)&p->d_lo, lo);
    if (rc2 == FD_OK && csc) rc2 = upload((int64_t **)&p->d_dst, dst);
    if (rc2 != FD_OK) return rc2;
    p->p_colptr.swap(pcp);
    p->p_rowval.swap(prv);
    p->built = true;
    return FD_OK;
}

static int check_pair(fd_hess_plan *plan, fd_objective *obj)
{
    FD_REQUIRE(plan && obj, FD_ERR_ARG, "NULL plan or objective");
    FD_REQUIRE(plan->M == obj->M && plan->N == obj->N, FD_ERR_SHAPE, "the objective is %lld x %lld, the plan %lld x %lld", (long long)obj->M,
               (long long)obj->N, (long long)plan->M, (long long)plan->N);
    FD_REQUIRE(plan->ctx == obj->ctx || plan->ctx->device == obj->ctx->device, FD_ERR_ARG, "the objective and the plan belong to different devices");
    return FD_OK;
}

static int rows_pass(fd_hess_plan *p, fd_objective *o, const void *x)
{
    void *fx = p->d_fx;
    long long M = p->M;
    void *args[] = {(void *)o->params.data(), (void *)&x, &fx, &M};
    FD_HIP_CHECK(hipModuleLaunchKernel(o->m->rows, fd_xcd_grid((M + 255) / 256), 1, 1, 256, 1, 1, 0, p->ctx->stream, args, nullptr));
    o->launches += 1;
    return FD_OK;
}

static int stage(double **buf, int64_t n)
{
    if (!*buf) FD_HIP_CHECK(hipMalloc((void **)buf, (size_t)std::max<int64_t>(n, 1) * sizeof(double)));
    return FD_OK;
}

}  // namespace fdjac

using namespace fdjac;

extern "C" {

int fd_objective_compile(fd_ctx *ctx, const char *source, const char *functor, const void *params, int64_t params_bytes, int64_t M, int64_t N,
                         fd_objective **out)
{
    if (int rc = require_device()) return rc;
    FD_REQUIRE(ctx && source && functor && out, FD_ERR_ARG, "NULL argument");
    *out = nullptr;
    FD_REQUIRE(M >= 1 && N >= 1 && M < ((int64_t)1 << 31) && N < ((int64_t)1 << 31), FD_ERR_ARG, "bad shape (1 <= M, N < 2^31)");
    FD_REQUIRE(params_bytes >= 0 && (params || params_bytes == 0), FD_ERR_ARG, "bad functor parameters");
    FD_REQUIRE(rtc_is_type_name(functor), FD_ERR_ARG, "functor must be a type name");
    FD_HIP_CHECK(hipSetDevice(ctx->device));
    rtc_log().clear();
    const std::string src = rtc_source("double", rtc_functor_text(source), std::string("FDOBJ_FUNCTOR ") + functor, kObjTail);
    const std::string key = std::to_string(ctx->device) + "\n" + src;
    ObjModule *m = g_obj_modules.acquire(key);
    if (!m) {
        m = new (std::nothrow) ObjModule();
        FD_REQUIRE(m, FD_ERR_NOMEM, "out of host memory");
        m->key = key;
        RtcResult r = rtc_compile(src, "fdjac_objective.hip", std::vector<char>(),
                                  {{"fd_obj_rows<double, fdobj_F>", true, &m->rows},
                                   {"fd_hess_entries<double, fdobj_F>", true, &m->hess},
                                   {"fd_grad_cols<double, 0, fdobj_F>", true, &m->grad[0]},
                                   {"fd_grad_cols<double, 1, fdobj_F>", true, &m->grad[1]}},
                                  {}, {{"fdobj_sizeof_f", &m->sizeof_f}});
        rtc_log() = r.log;
        m->mod = r.mod;
        if (r.status != RTC_OK) { delete m; return rtc_error(r, "objective"); }
        m = g_obj_modules.publish(m);
    }
    if (!((params_bytes == 0 && m->sizeof_f == 1) || (int64_t)m->sizeof_f == params_bytes)) {
        set_error("the functor %s is %u bytes, %lld bytes of parameters were given", functor, m->sizeof_f, (long long)params_bytes);
        g_obj_modules.release(m);
        return FD_ERR_ARG;
    }
    fd_objective *o = new (std::nothrow) fd_objective();
    if (!o) { g_obj_modules.release(m); set_error("out of host memory"); return FD_ERR_NOMEM; }
    o->ctx = ctx; o->m = m; o->M = M; o->N = N;
    o->params.assign(std::max<size_t>(m->sizeof_f, 16), 0);
    if (params_bytes > 0) memcpy(o->params.data(), params, (size_t)params_bytes);
    *out = o;
    return FD_OK;
}

int fd_objective_destroy(fd_objective *obj)
{
    if (int rc = require_device()) return rc;
    if (!obj) return FD_OK;
    (void)hipSetDevice(obj->ctx->device);
    (void)hipStreamSynchronize(obj->ctx->stream);
    g_obj_modules.release(obj->m);
    delete obj;
    return FD_OK;
}

int fd_objective_counts(fd_objective *obj, int64_t *launches)
{
    if (int rc = require_device()) return rc;
    FD_REQUIRE(obj && launches, FD_ERR_ARG, "NULL argument");
    *launches = obj->launches;
    return FD_OK;
}

int fd_hess_plan_create(fd_ctx *ctx, int64_t M, int64_t N, const void *colptr, const void *rowval, int idx_bytes, int idx_base, int dest,
                        int64_t band, fd_hess_plan **out)
{
    if (int rc = require_device()) return rc;
    FD_REQUIRE(ctx && out, FD_ERR_ARG, "NULL argument");
    *out = nullptr;
    FD_REQUIRE(M >= 1 && N >= 1 && M < ((int64_t)1 << 31) && N < ((int64_t)1 << 31), FD_ERR_ARG, "bad shape (1 <= M, N < 2^31)");
    FD_REQUIRE(dest == FD_HESS_DENSE || dest == FD_HESS_CSC || dest == FD_HESS_BANDED, FD_ERR_ARG, "dest must be FD_HESS_DENSE, _CSC or _BANDED");
    FD_REQUIRE((colptr == nullptr) == (rowval == nullptr), FD_ERR_ARG, "colptr and rowval: both given, or both NULL (dense support)");
    std::vector<int64_t> cp(N + 1, 0);
    std::vector<int32_t> rv;
    if (!colptr) {
        FD_REQUIRE(M * N < ((int64_t)1 << 40), FD_ERR_ARG, "dense support of %lld x %lld is too large", (long long)M, (long long)N);
        rv.resize((size_t)(M * N));
        for (int64_t j = 0; j < N; ++j) {
            cp[j + 1] = (j + 1) * M;
            for (int64_t r = 0; r < M; ++r) rv[(size_t)(j * M + r)] = (int32_t)r;
        }
    } else {
        FD_REQUIRE(idx_bytes == 4 || idx_bytes == 8, FD_ERR_ARG, "idx_bytes must be 4 or 8");
        FD_REQUIRE(idx_base == 0 || idx_base == 1, FD_ERR_ARG, "idx_base must be 0 or 1");
        auto at = [&](const void *a, int64_t k) -> int64_t { return idx_bytes == 8 ? ((const int64_t *)a)[k] : (int64_t)((const int32_t *)a)[k]; };
        const int64_t nnz = at(colptr, N) - idx_base;
        FD_REQUIRE(at(colptr, 0) == idx_base && nnz >= 0, FD_ERR_SHAPE, "colptr must start at idx_base and end at nnz + idx_base");
        rv.reserve((size_t)nnz);
        for (int64_t j = 0; j < N; ++j) {
            const int64_t a = at(colptr, j) - idx_base, b = at(colptr, j + 1) - idx_base;
            FD_REQUIRE(a <= b && b <= nnz, FD_ERR_SHAPE, "colptr is not monotone (column %lld)", (long long)j);
            const size_t c0 = rv.size();
            for (int64_t q = a; q < b; ++q) {
                const int64_t r = at(rowval, q) - idx_base;
                FD_REQUIRE(r >= 0 && r < M, FD_ERR_SHAPE, "rowval[%lld] = %lld out of range", (long long)q, (long long)(r + idx_base));
                rv.push_back((int32_t)r);
            }
            std::sort(rv.begin() + c0, rv.end());
            rv.erase(std::unique(rv.begin() + c0, rv.end()), rv.end());
            cp[j + 1] = (int64_t)rv.size();
        }
    }
    // P's half-bandwidth without P: the widest row of S
    std::vector<int32_t> rmin(M, INT32_MAX), rmax(M, -1);
    for (int64_t j = 0; j < N; ++j)
        for (int64_t q = cp[j]; q < cp[j + 1]; ++q) {
            rmin[rv[q]] = std::min<int32_t>(rmin[rv[q]], (int32_t)j);
            rmax[rv[q]] = std::max<int32_t>(rmax[rv[q]], (int32_t)j);
        }
    int64_t bw = 0;
    for (int64_t r = 0; r < M; ++r)
        if (rmax[r] >= 0) bw = std::max<int64_t>(bw, (int64_t)rmax[r] - rmin[r]);
    if (dest == FD_HESS_BANDED)
        FD_REQUIRE(band >= bw && band < N, FD_ERR_ARG, "band %lld is below the Hessian's half-bandwidth %lld (or not below N)", (long long)band, (long long)bw);
    FD_HIP_CHECK(hipSetDevice(ctx->device));
    fd_hess_plan *p = new (std::nothrow) fd_hess_plan();
    FD_REQUIRE(p, FD_ERR_NOMEM, "out of host memory");
    p->ctx = ctx; p->M = M; p->N = N; p->dest = dest; p->band = dest == FD_HESS_BANDED ? band : 0; p->bw = bw;
    p->s_colptr.swap(cp);
    p->s_rowval.swap(rv);
    int rc = upload((int64_t **)&p->d_scolptr, p->s_colptr);
    if (rc == FD_OK) rc = upload(&p->d_srowval, p->s_rowval);
    if (rc == FD_OK) rc = stage(&p->d_fx, M);
    if (rc != FD_OK) { fd_hess_plan_destroy(p); return rc; }
    *out = p;
    return FD_OK;
}

int fd_hess_plan_destroy(fd_hess_plan *p)
{
    if (int rc = require_device()) return rc;
    if (!p) return FD_OK;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    void *bufs[] = {p->d_scolptr, p->d_srowval, p->d_fx, p->d_ent_i, p->d_ent_j, p->d_rows, p->d_lo, p->d_dst, p->d_xstage, p->d_outstage};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    delete p;
    return FD_OK;
}

int fd_hess_plan_info(const fd_hess_plan *plan, int key, int64_t *value)
{
    if (int rc = require_device()) return rc;
    FD_REQUIRE(plan && value, FD_ERR_ARG, "NULL argument");
    fd_hess_plan *p = const_cast<fd_hess_plan *>(plan);      // (P is built on first use)
    if (key == FD_HESS_INFO_BANDWIDTH) { *value = p->bw; return FD_OK; }
    FD_REQUIRE(key >= FD_HESS_INFO_NNZ && key <= FD_HESS_INFO_OUT_LEN, FD_ERR_ARG, "unknown key %d", key);
    FD_HIP_CHECK(hipSetDevice(p->ctx->device));
    if (int rc = build_pattern(p)) return rc;
    *value = key == FD_HESS_INFO_NNZ ? (int64_t)p->p_rowval.size() : key == FD_HESS_INFO_UPPER ? p->nent : key == FD_HESS_INFO_LIST_LEN ? p->list_len
                                                                                                                                : hess_out_len(p);
    return FD_OK;
}

int fd_hess_plan_pattern(const fd_hess_plan *plan, int64_t *colptr_out, int64_t *rowval_out)
{
    if (int rc = require_device()) return rc;
    FD_REQUIRE(plan, FD_ERR_ARG, "NULL plan");
    fd_hess_plan *p = const_cast<fd_hess_plan *>(plan);
    FD_HIP_CHECK(hipSetDevice(p->ctx->device));
    if (int rc = build_pattern(p)) return rc;
    if (colptr_out) memcpy(colptr_out, p->p_colptr.data(), p->p_colptr.size() * sizeof(int64_t));
    if (rowval_out)
        for (size_t k = 0; k < p->p_rowval.size(); ++k) rowval_out[k] = p->p_rowval[k];
    return FD_OK;
}

int fd_hessian_async(fd_hess_plan *p, fd_objective *o, const void *x, double relstep, double absstep, void *H)
{
    if (int rc = require_device()) return rc;
    if (int rc = check_pair(p, o)) return rc;
    FD_REQUIRE(x, FD_ERR_ARG, "NULL x or H");
    FD_HIP_CHECK(hipSetDevice(p->ctx->device));
    if (int rc = build_pattern(p)) return rc;
    FD_REQUIRE(H || hess_out_len(p) == 0, FD_ERR_ARG, "NULL x or H");      // (a CSC destination of no entries has no address)
    if (!(relstep > 0)) relstep = 0x1p-13;                       // default_relstep(Val(:hcentral), Float64) = eps(Float64)^(1/4)
    if (absstep < 0) absstep = relstep;
    hipStream_t s = p->ctx->stream;
    const int64_t N = p->N;
    if (p->dest == FD_HESS_DENSE) {
        FD_HIP_CHECK(hipMemsetAsync(H, 0, (size_t)(N * N) * sizeof(double), s));
    } else if (p->dest == FD_HESS_BANDED) {
        const int64_t w = 2 * p->band + 1;
        if (p->band_full && 2 * p->band < N) {      // (only the corner columns hold out-of-matrix slots)
            FD_HIP_CHECK(hipMemsetAsync(H, 0, (size_t)(w * p->band) * sizeof(double), s));
            FD_HIP_CHECK(hipMemsetAsync((double *)H + w * (N - p->band), 0, (size_t)(w * p->band) * sizeof(double), s));
        } else {
            FD_HIP_CHECK(hipMemsetAsync(H, 0, (size_t)(w * N) * sizeof(double), s));
        }
    }
    if (p->nent == 0) return FD_OK;      // (no row reads anything: H = 0)
    if (int rc = rows_pass(p, o, x)) return rc;
    fd_hess_desc d;
    d.ent_i = p->d_ent_i; d.ent_j = p->d_ent_j; d.lo = p->d_lo; d.rows = p->d_rows; d.dst = p->d_dst; d.out = H;
    d.nent = p->nent; d.ndiag = p->ndiag; d.N = N; d.dest = p->dest; d.band = (int)p->band;
    const double *fx = p->d_fx;
    void *args[] = {(void *)o->params.data(), (void *)&x, (void *)&fx, &relstep, &absstep, &d};
    FD_HIP_CHECK(hipModuleLaunchKernel(o->m->hess, fd_xcd_grid((p->nent + 255) / 256), 1, 1, 256, 1, 1, 0, s, args, nullptr));
    o->launches += 1;
    return FD_OK;
}

int fd_hessian(fd_hess_plan *p, fd_objective *o, const void *x, int x_kind, double relstep, double absstep, void *H, int out_kind)
{
    if (int rc = require_device()) return rc;
    if (int rc = check_pair(p, o)) return rc;
    FD_REQUIRE(x, FD_ERR_ARG, "NULL x or H");
    FD_REQUIRE((x_kind == FD_HOST || x_kind == FD_DEVICE) && (out_kind == FD_HOST || out_kind == FD_DEVICE), FD_ERR_ARG, "bad memory kind");
    FD_HIP_CHECK(hipSetDevice(p->ctx->device));
    if (int rc = build_pattern(p)) return rc;
    FD_REQUIRE(H || hess_out_len(p) == 0, FD_ERR_ARG, "NULL x or H");
    hipStream_t s = p->ctx->stream;
    const void *xd = x;
    if (x_kind == FD_HOST) {
        if (int rc = stage(&p->d_xstage, p->N)) return rc;
        FD_HIP_CHECK(hipMemcpyAsync(p->d_xstage, x, (size_t)p->N * sizeof(double), hipMemcpyHostToDevice, s));
        xd = p->d_xstage;
    }
    const int64_t n = hess_out_len(p);
    void *Hd = H;
    if (out_kind == FD_HOST) {
        if (p->outstage_n < n && p->d_outstage) { (void)hipFree(p->d_outstage); p->d_outstage = nullptr; }
        if (int rc = stage(&p->d_outstage, n)) return rc;
        p->outstage_n = std::max<int64_t>(p->outstage_n, n);
        Hd = p->d_outstage;
    }
    if (int rc = fd_hessian_async(p, o, xd, relstep, absstep, Hd)) return rc;
    if (out_kind == FD_HOST && n > 0) FD_HIP_CHECK(hipMemcpyAsync(H, Hd, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    FD_HIP_CHECK(hipStreamSynchronize(s));
    return FD_OK;
}

int fd_gradient_async(fd_hess_plan *p, fd_objective *o, const void *x, int fdtype, double relstep, double absstep, double dir, void *df)
{
    if (int rc = require_device()) return rc;
    if (int rc = check_pair(p, o)) return rc;
    FD_REQUIRE(x && df, FD_ERR_ARG, "NULL x or df");
    FD_REQUIRE(fdtype != FD_COMPLEX, FD_ERR_UNSUPPORTED, "the complex-step gradient of an objective is not supported (forward or central)");
    FD_REQUIRE(fdtype == FD_FORWARD || fdtype == FD_CENTRAL, FD_ERR_ARG, "fdtype must be FD_FORWARD or FD_CENTRAL");
    FD_HIP_CHECK(hipSetDevice(p->ctx->device));
    const double e = std::numeric_limits<double>::epsilon();     // default_relstep, src/epsilons.jl:133-144
    if (!(relstep > 0)) relstep = fdtype == FD_FORWARD ? std::sqrt(e) : std::cbrt(e);
    if (absstep < 0) absstep = relstep;
    const int central = fdtype == FD_CENTRAL ? 1 : 0;
    if (!central)
        if (int rc = rows_pass(p, o, x)) return rc;
    const double *fx = central ? nullptr : p->d_fx;
    const long long *cp = p->d_scolptr;
    const int *rv = p->d_srowval;
    long long N = p->N;
    void *args[] = {(void *)o->params.data(), (void *)&x, (void *)&fx, &relstep, &absstep, &dir, (void *)&cp, (void *)&rv, &df, &N};
    FD_HIP_CHECK(hipModuleLaunchKernel(o->m->grad[central], fd_xcd_grid((N + 255) / 256), 1, 1, 256, 1, 1, 0, p->ctx->stream, args, nullptr));
    o->launches += 1;
    return FD_OK;
}

int fd_gradient(fd_hess_plan *p, fd_objective *o, const void *x, int x_kind, int fdtype, double relstep, double absstep, double dir, void *df,
                int out_kind)
{
    if (int rc = require_device()) return rc;
    if (int rc = check_pair(p, o)) return rc;
    FD_REQUIRE(x && df, FD_ERR_ARG, "NULL x or df");
    FD_REQUIRE((x_kind == FD_HOST || x_kind == FD_DEVICE) && (out_kind == FD_HOST || out_kind == FD_DEVICE), FD_ERR_ARG, "bad memory kind");
    FD_REQUIRE(fdtype != FD_COMPLEX, FD_ERR_UNSUPPORTED, "the complex-step gradient of an objective is not supported (forward or central)");
    FD_HIP_CHECK(hipSetDevice(p->ctx->device));
    hipStream_t s = p->ctx->stream;
    const void *xd = x;
    if (x_kind == FD_HOST) {
        if (int rc = stage(&p->d_xstage, p->N)) return rc;
        FD_HIP_CHECK(hipMemcpyAsync(p->d_xstage, x, (size_t)p->N * sizeof(double), hipMemcpyHostToDevice, s));
        xd = p->d_xstage;
    }
    void *dd = df;
    if (out_kind == FD_HOST) {
        if (p->outstage_n < p->N && p->d_outstage) { (void)hipFree(p->d_outstage); p->d_outstage = nullptr; }
        if (int rc = stage(&p->d_outstage, p->N)) return rc;
        p->outstage_n = std::max<int64_t>(p->outstage_n, p->N);
        dd = p->d_outstage;
    }
    if (int rc = fd_gradient_async(p, o, xd, fdtype, relstep, absstep, dir, dd)) return rc;
    if (out_kind == FD_HOST) FD_HIP_CHECK(hipMemcpyAsync(df, dd, (size_t)p->N * sizeof(double), hipMemcpyDeviceToHost, s));
    FD_HIP_CHECK(hipStreamSynchronize(s));
    return FD_OK;
}

}  // extern "C"
