// Shared by the matrix-free consumers (fdjac_jfnk.hip, fdjac_jftr.hip; Float64 only): what both handles hold and the one way from them
// into the finite-difference JVP (jvp_enqueue through JvpHooks, fdjac_internal.h).  Create and destroy are csc_handle_create /
// csc_handle_destroy (fdjac_csc_common.h), as for the consumers on stored matrices.  The device side of the shared dot is fdjac_dotx.h.
#pragma once
#include "fdjac_csc_common.h"
#include "fdjac_dotx.h"

namespace fdjac {

// the range checks of a create, before the first dereference of ctx (the CPU tests send a context that is never dereferenced)
inline int mf_check_args(const fd_ctx *ctx, int64_t N, int fdtype)
{
    FD_REQUIRE(ctx != nullptr, FD_ERR_ARG, "NULL argument");
    FD_REQUIRE(N >= 1 && N <= (int64_t)0x7FFFFFFF - kCsVecTile, FD_ERR_SHAPE, "N = %lld (1 .. 2^31 - 1025)", (long long)N);
    if (fdtype != FD_FORWARD && fdtype != FD_CENTRAL) {
        set_error("finite_difference_jvp doesn't support :complex-mode finite diff");
        return FD_ERR_UNSUPPORTED;
    }
    return FD_OK;
}

// What fd_jfnk_solver and fd_jftr derive from.  The destructor frees (the stream has been synchronised; a half-built object is fine): a
// consumer with buffers of its own frees them in its own.
struct MfHandle {
    fd_ctx *ctx = nullptr;
    int64_t N = 0, ld = 0;             // ld: N rounded up to 32 (every vector of d_vec starts on a pair)
    int fdtype = FD_FORWARD;
    CscSolveState S;
    fd_jvp_plan *jp = nullptr;
    double *d_vec = nullptr;           // the consumer's vectors and, last, its own f(x): ld doubles each
    const double *d_diag = nullptr;    // the caller's diagonal, or NULL
    double relstep = -1.0, absstep = -1.0, dir = 1.0;
    int64_t base_evaluations = 0;      // launches of f! for f(x)
    MfHandle() = default;
    MfHandle(const MfHandle &) = delete;
    ~MfHandle()
    {
        S.free();
        if (jp) (void)fd_jvp_plan_destroy(jp);
        if (d_vec) (void)hipFree(d_vec);
    }
    // the JVP plan, nvec_slots vectors, the state of a solve with nscal scalars and npart partial sums
    int init(fd_ctx *ctx_, const char *who, int64_t N_, int fdtype_, int nvec_slots, int nscal, int64_t npart)
    {
        const int ra = mf_check_args(ctx_, N_, fdtype_);
        if (ra != FD_OK) return ra;
        FD_HIP_CHECK(hipSetDevice(ctx_->device));
        ctx = ctx_; N = N_; ld = (N_ + 31) / 32 * 32; fdtype = fdtype_;
        const int rc = fd_jvp_plan_create(ctx, N, N, fdtype, &jp);
        if (rc != FD_OK) return rc;
        CSC_TRY(who, hipMalloc((void **)&d_vec, sizeof(double) * (size_t)nvec_slots * (size_t)ld));
        return S.create(who, ctx->stream, nscal, npart);
    }
    double *vec(int k) const { return d_vec + (size_t)k * (size_t)ld; }
    // f(x) once per call in the forward arm without f_in: one launch of f! into vec(slot).  fin: the subtrahend of the forward arm (NULL
    // in the central arm); own: it is the consumer's own f(x)
    int base(fd_f_launch f, void *fctx, const double *x, const double *f_in, int slot, const double **fin, bool *own)
    {
        *fin = nullptr; *own = false;
        if (fdtype != FD_FORWARD) return FD_OK;
        if (f_in) { *fin = f_in; return FD_OK; }
        double *fx = vec(slot);
        const int rc = f(fctx, fx, x, 1, N, ld, 0, N, 0, (void *)ctx->stream);
        FD_REQUIRE(rc == 0, FD_ERR_CALLBACK, "f! launcher returned %d", rc);
        base_evaluations += 1;
        *fin = fx; *own = true;
        return FD_OK;
    }
    // the JVP of (x, v) with the consumer's steps, closed by close(user, ...) where k_jvp_diff stood; have_partials: the caller's kernel
    // has left the partial sums of dot(x, v) in jp->d_partial (fdjac_dotx.h)
    int enqueue(fd_f_launch f, void *fctx, const double *x, const double *v, const double *fin, bool own, double *out, bool have_partials, void *user,
                int (*close)(void *, const double *, const double *, const double *, int))
    {
        JvpHooks hk = {have_partials, own, user, close};
        return jvp_enqueue_hooked(jp, f, fctx, x, v, fin, relstep, absstep, dir, out, &hk);
    }
    int set_steps(double relstep_, double absstep_, double dir_)
    {
        relstep = relstep_; absstep = absstep_; dir = dir_;
        return FD_OK;
    }
    int set_lazy(fd_f_launch_lazy_jvp lazy, int caps)
    {
        FD_REQUIRE(lazy != nullptr || caps == 0, FD_ERR_ARG, "no lazy launcher installed");
        const int rc = fd_jvp_plan_set_lazy_f(jp, lazy);
        return rc != FD_OK ? rc : fd_jvp_plan_set_lazy_caps(jp, caps);
    }
};

}  // namespace fdjac
