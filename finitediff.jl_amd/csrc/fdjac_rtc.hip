// The library's ONE runtime compiler: everything a caller hands over as text or bitcode -- row functors, separable terms, linked bitcode
// (fdjac_jit.hip), objectives (fdjac_hessian.hip) -- becomes a loaded module here.  The translation unit is the embedded
// include/fdjac_device.h, the element type, the caller's part and a kernel tail; it is compiled with hiprtc for gfx950,
// -ffp-contract=off as the library itself is built (the reference never fuses a*b+c), and its kernels are found by their lowered names.
//
// hiprtc is bound at run time (dlopen), like RCCL: libfdjac loads on boxes without it and the compiling entry points say so.
#include <dlfcn.h>
#include <hip/hiprtc.h>

#include <mutex>

#include "fdjac_internal.h"

namespace fdjac {

static const char kDeviceHeader[] =
#include "fdjac_device_h.inc"
    ;

static thread_local std::string t_log;
std::string &rtc_log() { return t_log; }
static thread_local int t_store_launch = 0;

struct Hiprtc {
    void *handle = nullptr;
    decltype(&hiprtcCreateProgram) CreateProgram = nullptr;
    decltype(&hiprtcDestroyProgram) DestroyProgram = nullptr;
    decltype(&hiprtcCompileProgram) CompileProgram = nullptr;
    decltype(&hiprtcAddNameExpression) AddNameExpression = nullptr;
    decltype(&hiprtcGetLoweredName) GetLoweredName = nullptr;
    decltype(&hiprtcGetProgramLogSize) GetProgramLogSize = nullptr;
    decltype(&hiprtcGetProgramLog) GetProgramLog = nullptr;
    decltype(&hiprtcGetCodeSize) GetCodeSize = nullptr;
    decltype(&hiprtcGetCode) GetCode = nullptr;
    decltype(&hiprtcGetErrorString) GetErrorString = nullptr;
    // linking a caller's LLVM bitcode in (fd_f_link_rows_bitcode): optional -- an older hiprtc without them serves source functors only
    decltype(&hiprtcGetBitcodeSize) GetBitcodeSize = nullptr;
    decltype(&hiprtcGetBitcode) GetBitcode = nullptr;
    decltype(&hiprtcLinkCreate) LinkCreate = nullptr;
    decltype(&hiprtcLinkAddData) LinkAddData = nullptr;
    decltype(&hiprtcLinkComplete) LinkComplete = nullptr;
    decltype(&hiprtcLinkDestroy) LinkDestroy = nullptr;
};

// (a failure is reported through set_error and tried again by the next call)
static const Hiprtc *hiprtc()
{
    static Hiprtc g_rtc;
    static std::mutex g_mutex;
    std::lock_guard<std::mutex> lock(g_mutex);
    if (g_rtc.handle) return &g_rtc;
    const char *env = getenv("FDJAC_HIPRTC_LIB");
    const char *names[] = {env && *env ? env : "libhiprtc.so", "libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
    void *h = nullptr;
    for (const char *n : names)
        if (!h) h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
        set_error("hiprtc not found (tried libhiprtc.so, /opt/rocm/lib; set FDJAC_HIPRTC_LIB): %s", dlerror());
        return nullptr;
    }
    Hiprtc r;
    r.handle = h;
#define FD_SYM(field, name)                                            \
    r.field = (decltype(r.field))dlsym(h, name);                       \
    if (!r.field) {                                                    \
        set_error("hiprtc symbol %s missing", name);                   \
        return nullptr;                                                \
    }
    FD_SYM(CreateProgram, "hiprtcCreateProgram")
    FD_SYM(DestroyProgram, "hiprtcDestroyProgram")
    FD_SYM(CompileProgram, "hiprtcCompileProgram")
    FD_SYM(AddNameExpression, "hiprtcAddNameExpression")
    FD_SYM(GetLoweredName, "hiprtcGetLoweredName")
    FD_SYM(GetProgramLogSize, "hiprtcGetProgramLogSize")
    FD_SYM(GetProgramLog, "hiprtcGetProgramLog")
    FD_SYM(GetCodeSize, "hiprtcGetCodeSize")
    FD_SYM(GetCode, "hiprtcGetCode")
    FD_SYM(GetErrorString, "hiprtcGetErrorString")
#undef FD_SYM
    r.GetBitcodeSize = (decltype(r.GetBitcodeSize))dlsym(h, "hiprtcGetBitcodeSize");
    r.GetBitcode = (decltype(r.GetBitcode))dlsym(h, "hiprtcGetBitcode");
    r.LinkCreate = (decltype(r.LinkCreate))dlsym(h, "hiprtcLinkCreate");
    r.LinkAddData = (decltype(r.LinkAddData))dlsym(h, "hiprtcLinkAddData");
    r.LinkComplete = (decltype(r.LinkComplete))dlsym(h, "hiprtcLinkComplete");
    r.LinkDestroy = (decltype(r.LinkDestroy))dlsym(h, "hiprtcLinkDestroy");
    g_rtc = r;
    return &g_rtc;
}

bool rtc_is_type_name(const char *s)
{
    for (const char *c = s; *c; ++c)
        if (!((*c >= 'a' && *c <= 'z') || (*c >= 'A' && *c <= 'Z') || (*c >= '0' && *c <= '9') || *c == '_' || *c == ':' || *c == '<' || *c == '>' || *c == ',' ||
              *c == ' '))
            return false;
    return true;
}

std::string rtc_source(const char *real, const std::string &body, const std::string &define, const std::string &tail)
{
    std::string src;      // (hiprtc declares the HIP runtime itself: no include)
    src += kDeviceHeader;
    src += "\ntypedef ";
    src += real;
    src += " real_t;\n";
    src += body;
    src += "\n#define ";
    src += define;
    src += "\n";
    src += tail;
    return src;
}

// a compiled program as a loaded module.  bitcode empty: the program's code object; else the program (compiled with -fgpu-rdc) and the
// caller's bitcode linked into one code object first (hiprtcLink*, LLVM bitcode inputs: the caller's row function is inlined into the
// kernels like a source functor's call operator)
static const char *const kOpts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-math-errno", "-fgpu-rdc"};
static RtcStatus load_program(const Hiprtc *R, hiprtcProgram prog, const std::vector<char> &bitcode, hipModule_t *mod, std::string *why)
{
    hipError_t e = hipErrorUnknown;
    if (bitcode.empty()) {
        size_t cs = 0;
        std::vector<char> code;
        if (R->GetCodeSize(prog, &cs) != HIPRTC_SUCCESS || cs == 0) { *why = "hiprtcGetCodeSize failed"; return RTC_LOAD; }
        code.resize(cs);
        if (R->GetCode(prog, code.data()) != HIPRTC_SUCCESS) { *why = "hiprtcGetCode failed"; return RTC_LOAD; }
        e = hipModuleLoadData(mod, code.data());
    } else {
        if (!R->GetBitcode || !R->GetBitcodeSize || !R->LinkCreate || !R->LinkAddData || !R->LinkComplete || !R->LinkDestroy) { *why = "this hiprtc has no link interface"; return RTC_LINK; }
        size_t bs = 0;
        if (R->GetBitcodeSize(prog, &bs) != HIPRTC_SUCCESS || bs == 0) { *why = "hiprtcGetBitcodeSize failed"; return RTC_LINK; }
        std::vector<char> glue(bs), user(bitcode);
        if (R->GetBitcode(prog, glue.data()) != HIPRTC_SUCCESS) { *why = "hiprtcGetBitcode failed"; return RTC_LINK; }
        hiprtcLinkState ls = nullptr;
        if (R->LinkCreate(0, nullptr, nullptr, &ls) != HIPRTC_SUCCESS) { *why = "hiprtcLinkCreate failed"; return RTC_LINK; }
        void *bin = nullptr;
        size_t sz = 0;
        hiprtcResult r = R->LinkAddData(ls, HIPRTC_JIT_INPUT_LLVM_BITCODE, glue.data(), glue.size(), "fdjac kernels", 0, nullptr, nullptr);
        if (r == HIPRTC_SUCCESS) r = R->LinkAddData(ls, HIPRTC_JIT_INPUT_LLVM_BITCODE, user.data(), user.size(), "caller's row function", 0, nullptr, nullptr);
        if (r == HIPRTC_SUCCESS) r = R->LinkComplete(ls, &bin, &sz);
        const bool linked = r == HIPRTC_SUCCESS && bin && sz;
        if (linked) e = hipModuleLoadData(mod, bin);
        else *why = std::string("linking the caller's bitcode failed (") + R->GetErrorString(r) + "): does it define fdjac_user_row (and fdjac_user_row_c for the complex step) for gfx950?";
        (void)R->LinkDestroy(ls);
        if (!linked) return RTC_LINK;
    }
    if (e != hipSuccess) *why = hipGetErrorString(e);
    return e == hipSuccess ? RTC_OK : RTC_LOAD;
}

RtcResult rtc_compile(const std::string &src, const char *program, const std::vector<char> &bitcode, const std::vector<RtcName> &names,
                      const std::vector<RtcKernel> &kernels, const std::vector<RtcGlobal> &globals)
{
    RtcResult out;
    const Hiprtc *R = hiprtc();
    if (!R) { out.status = RTC_UNAVAILABLE; return out; }
    hiprtcProgram prog = nullptr;
    hiprtcResult rr = R->CreateProgram(&prog, src.c_str(), program, 0, nullptr, nullptr);
    if (rr != HIPRTC_SUCCESS) { out.status = RTC_CREATE; out.why = R->GetErrorString(rr); return out; }
    for (const RtcName &n : names) (void)R->AddNameExpression(prog, n.expr.c_str());
    rr = R->CompileProgram(prog, bitcode.empty() ? 5 : 6, kOpts);
    size_t ls = 0;
    if (R->GetProgramLogSize(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
        out.log.resize(ls);
        (void)R->GetProgramLog(prog, &out.log[0]);
    }
    std::vector<std::string> low(names.size());      // (the lowered names belong to the program: copied before it goes)
    if (rr != HIPRTC_SUCCESS) {
        out.status = RTC_COMPILE;
        out.why = R->GetErrorString(rr);
    } else {
        for (size_t k = 0; k < names.size(); ++k) {
            const char *ln = nullptr;
            if (R->GetLoweredName(prog, names[k].expr.c_str(), &ln) == HIPRTC_SUCCESS && ln) low[k] = ln;
        }
        out.status = load_program(R, prog, bitcode, &out.mod, &out.why);
    }
    (void)R->DestroyProgram(&prog);
    if (out.status == RTC_OK) {
        hipError_t e = hipSuccess;
        for (size_t k = 0; k < names.size(); ++k) {
            const hipError_t ek = low[k].empty() ? hipErrorNotFound : hipModuleGetFunction(names[k].fn, out.mod, low[k].c_str());
            if (ek != hipSuccess) *names[k].fn = nullptr;      // (an optional form is an optimisation: its caller has another way)
            if (ek != hipSuccess && names[k].required && e == hipSuccess) e = ek;
        }
        for (const RtcKernel &k : kernels)
            if (e == hipSuccess) e = hipModuleGetFunction(k.fn, out.mod, k.name);
        for (const RtcGlobal &g : globals) {
            hipDeviceptr_t dp = nullptr;
            size_t bytes = 0;
            if (e == hipSuccess) e = hipModuleGetGlobal(&dp, &bytes, out.mod, g.name);
            if (e == hipSuccess) e = hipMemcpy(g.value, dp, sizeof(unsigned), hipMemcpyDeviceToHost);
        }
        if (e != hipSuccess) { out.status = RTC_LOAD; out.why = hipGetErrorString(e); }
    }
    if (out.status == RTC_LINK) out.log += out.why;
    if (out.status != RTC_OK) {
        for (const RtcName &n : names) *n.fn = nullptr;
        for (const RtcKernel &k : kernels) *k.fn = nullptr;
        if (out.mod) (void)hipModuleUnload(out.mod);
        out.mod = nullptr;
    }
    (void)hipGetLastError();
    return out;
}

int rtc_error(const RtcResult &r, const char *what)
{
    switch (r.status) {
    case RTC_OK: return FD_OK;
    case RTC_UNAVAILABLE: return FD_ERR_UNSUPPORTED;      // (the binding has said what is missing)
    case RTC_CREATE: set_error("hiprtcCreateProgram failed: %s", r.why.c_str()); return FD_ERR_HIP;
    case RTC_COMPILE:
        set_error("compiling the %s failed (%s); the compiler's messages: fd_f_compile_log().  First lines: %.300s", what, r.why.c_str(), r.log.c_str());
        return FD_ERR_ARG;
    case RTC_LINK: set_error("%s", r.why.c_str()); return FD_ERR_ARG;
    default: set_error("loading the compiled %s failed: %s", what, r.why.c_str()); return FD_ERR_HIP;
    }
}

}  // namespace fdjac

extern "C" const char *fd_f_compile_log(void) { return fdjac::t_log.c_str(); }
extern "C" int *fdjac_store_launch_note_(void) { return &fdjac::t_store_launch; }
