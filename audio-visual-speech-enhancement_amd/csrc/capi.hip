// libavse C-ABI (include/avse.h): contexts and their options, the device copies of the librosa-equivalent tables
// (spec_tables.cpp) and of the evaluate stage's (eval_tables.cpp), and the audio, preprocess and evaluate entry points.
// The weights are weights.hip's, the forward forward.hip's.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>

#include "ctx.h"
#include "eval_tables.h"
#include "spec_tables.h"

namespace avse {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

int ensure_lds_attr(const void* fn, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;   // (kernel, device)
    int dev = 0;
    AVSE_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({fn, dev})) return 0;
    AVSE_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.insert({fn, dev});
    return 0;
}

int fail(int code, const std::string& msg) {
    set_error(msg);
    return code;
}

int ctx_device_index(const avse_ctx* c) { return c->device; }
}  // namespace avse

using namespace avse;

// the host-only tables' element types are uploaded as the HIP vector types the kernels read
static_assert(sizeof(Cplx) == sizeof(float2) && offsetof(Cplx, im) == offsetof(float2, y), "Cplx must match float2");
static_assert(sizeof(MelBin) == sizeof(float4) && offsetof(MelBin, j0) == offsetof(float4, z), "MelBin must match float4");

// avse_ctx_set_option names (and the AVSE_* variables that initialise them at avse_ctx_create)
struct OptionName {
    const char* name;
    const char* env;
    int Options::*field;
};
const OptionName kOptionNames[] = {
    {"no_gemm", "AVSE_NO_GEMM", &Options::no_gemm},
    {"no_audenc", "AVSE_NO_AUDENC", &Options::no_audenc},
    {"no_dechead", "AVSE_NO_DECHEAD", &Options::no_dechead},
    {"no_dectail", "AVSE_NO_DECTAIL", &Options::no_dectail},
    {"unfused_tail", "AVSE_UNFUSED_TAIL", &Options::unfused_tail},
    {"no_halo", "AVSE_NO_HALO", &Options::no_halo},
    {"mfma32", "AVSE_MFMA32", &Options::mfma32},
    {"serial", "AVSE_SERIAL", &Options::serial},
    {"graph", "AVSE_GRAPH", &Options::graph},
    {"gemm_ksplit_cap", "AVSE_GEMM_KSPLIT", &Options::gemm_ksplit_cap},
    {"dense_istft", "AVSE_DENSE_ISTFT", &Options::dense_istft},
    {"no_act_scale", "AVSE_NO_ACT_SCALE", &Options::no_act_scale},
    {"no_win", "AVSE_NO_WIN", &Options::no_win},
    {"no_v1p", "AVSE_NO_V1P", &Options::no_v1p},
    {"no_a1valu", "AVSE_NO_A1VALU", &Options::no_a1valu},
    {"no_planar", "AVSE_NO_PLANAR", &Options::no_planar},
    {"four_products", "AVSE_FOUR_PRODUCTS", &Options::four_products},
    {"side_prio", "AVSE_SIDE_PRIO", &Options::side_prio},
};

namespace {

const OptionName* find_option(const char* name) {
    for (const OptionName& o : kOptionNames)
        if (std::strcmp(o.name, name) == 0) return &o;
    return nullptr;
}

// Uploads a ragged batch's rows and item table (ragged_geom.h) into the preprocess scratch on `s` and points *d at
// them.  The scratch and the pinned staging copy grow outside a stream capture only.
int upload_ragged(avse_ctx* c, const RaggedGeom& g, hipStream_t s, RaggedDev* d) {
    const size_t ub = sizeof(RaggedUtt) * g.utt.size(), ib = sizeof(RaggedItem) * g.items.size();
    const size_t need = ub + ib;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (s) AVSE_HIP_CHECK(hipStreamIsCapturing(s, &cs));
    const bool capturing = cs != hipStreamCaptureStatusNone;
    if (int rc = grow(c->prep, need, s, "preprocess scratch")) return rc;
    if (!capturing && c->ragged_done) AVSE_HIP_CHECK(hipEventSynchronize(c->ragged_done));   // the last upload has read it
    if (int rc = grow(c->ragged_host, need, s, "ragged tables")) return rc;
    if (!c->ragged_done) AVSE_HIP_CHECK(hipEventCreateWithFlags(&c->ragged_done, hipEventDisableTiming));
    std::memcpy(c->ragged_host, g.utt.data(), ub);
    std::memcpy(c->ragged_host + ub, g.items.data(), ib);
    AVSE_HIP_CHECK(hipMemcpyAsync(c->prep, c->ragged_host, need, hipMemcpyHostToDevice, s));
    if (!capturing) AVSE_HIP_CHECK(hipEventRecord(c->ragged_done, s));
    d->utt = reinterpret_cast<const RaggedUtt*>(c->prep.p.get());
    d->items = reinterpret_cast<const RaggedItem*>(c->prep + ub);
    d->n_utt = (int)g.utt.size();
    d->n_items = (int)g.items.size();
    return 0;
}

// allocation + copy of a host table into `out` (D: the device-side element type of the same layout)
template <typename D, typename T>
int table_to_device(const std::vector<T>& h, Owned<D>& out) {
    static_assert(sizeof(D) == sizeof(T), "element layout");
    AVSE_HIP_CHECK(out.alloc(sizeof(T) * h.size()));
    AVSE_HIP_CHECK(hipMemcpy(out, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return 0;
}

int ensure_spec_tables(avse_ctx* c, int sr, int n_fft, int n_mels, double fmin, double fmax) {
    return build_spec_tables(c->spec, sr, n_fft, n_mels, fmin, fmax);
}

int ensure_istft_tables(avse_ctx* c, int sr, int n_fft, int n_mels, double fmin, double fmax) {
    return build_istft_tables(c->istft, sr, n_fft, n_mels, fmin, fmax);
}

// the resampling filter for sr -> 10 kHz, STOI's window / bands / twiddles and the segmental SNR's window
// any_rate (AVSE_EVAL_ANY_RATE): a rate with max(up, down) > 24 gets its real filter, by phase; such an entry and the
// default call's entry of the same rate (the copy filter) are different entries of the cache
int ensure_eval_tables(avse_ctx* c, int sr, bool any_rate, hipStream_t s, const EvalTables** out) {
    int up, down;
    eval_ratio(sr, &up, &down);
    const bool big = any_rate && std::max(up, down) > kEvalMaxRatio;
    for (const EvalTables& have : c->eval)
        if (have.sr == sr && have.big == big) {
            *out = &have;
            return 0;
        }
    // building and uploading tables allocates and copies: like the scratch, never inside a capture
    if (int rc = not_capturing(s, "the tables of this sample rate would be built while the stream is being captured: run "
                                  "one call with this rate before the capture"))
        return rc;
    EvalTables& t = c->eval[c->eval_next];
    c->eval_next = (c->eval_next + 1) % 4;
    *out = &t;
    t = EvalTables();
    const int win = seg_snr_window(sr);
    // a rate STOI is not computed for gets the copy filter: the resampler does not run
    const bool stoi = big || std::max(up, down) <= kEvalMaxRatio;
    const std::vector<double> taps = stoi ? resample_taps(up, down) : resample_taps(1, 1);
    if (big) {
        if (int rc = table_to_device(resample_taps_by_phase(taps, up), t.ptaps)) return rc;
    } else {
        if (int rc = table_to_device(taps, t.taps)) return rc;
    }
    if (int rc = table_to_device(hann_inner(kStoiFrame), t.W)) return rc;
    if (int rc = table_to_device(stoi_twiddle(), t.twid)) return rc;
    if (int rc = table_to_device(hann_inner(win), t.segw)) return rc;
    if (int rc = table_to_device(stoi_bands(), t.bands)) return rc;
    t.up = up; t.down = down; t.H = ((int)taps.size() - 1) / 2; t.win = win;
    t.sr = sr;
    t.big = big;
    return 0;
}

// The parameter checks of avse_spectrogram and its ragged form, in the order the C-ABI reports them.  n_samples: the
// uniform form's length; NULL for the ragged form, whose lengths its RaggedGeom checks per utterance.
int spec_check(bool pointers, int64_t n_utt, const int64_t* n_samples, int sr, int n_fft, int hop, int n_mels, int pad_mode,
               int frames_per_slice) {
    if (!pointers) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n_utt < 0 || (n_samples && *n_samples <= 0) || sr <= 0 || hop <= 0 || n_fft < 2)
        return fail(AVSE_ERR_INVALID, "bad spectrogram geometry");
    if (n_fft > 2048) return fail(AVSE_ERR_UNSUPPORTED, "n_fft > 2048 not supported");
    if (n_mels < 1 || n_mels > 80) return fail(AVSE_ERR_UNSUPPORTED, "n_mels must be in [1, 80]");
    if (pad_mode != AVSE_PAD_REFLECT && pad_mode != AVSE_PAD_CONSTANT) return fail(AVSE_ERR_INVALID, "bad pad_mode");
    if (n_samples && pad_mode == AVSE_PAD_REFLECT && *n_samples <= n_fft / 2)
        return fail(AVSE_ERR_INVALID, "reflect padding needs n_samples > n_fft/2");
    if (frames_per_slice < 0) return fail(AVSE_ERR_INVALID, "frames_per_slice < 0");
    return 0;
}

// The tables and the per-utterance max words of a checked spectrogram call, and its launch arguments but for the
// lengths: n_samples, n_frames and n_slices stay 0 (the uniform form sets them; per utterance in a ragged batch).
int spec_args(avse_ctx* c, const float* sig, int64_t n_utt, int sr, int n_fft, int hop, int n_mels, float fmin, float fmax,
              float amin, float top_db, int pad_mode, int frames_per_slice, float* mel_db, float* stft_ri, hipStream_t s,
              SpecArgs* out) {
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = ensure_spec_tables(c, sr, n_fft, n_mels, fmin, fmax)) return rc;
    if (int rc = grow(c->umax, sizeof(unsigned) * (size_t)n_utt, s, "spectrogram scratch")) return rc;
    SpecArgs a;
    std::memset(&a, 0, sizeof(a));
    a.sig = sig; a.mel_db = mel_db; a.stft_ri = stft_ri;
    a.n_utt = n_utt; a.n_fft = n_fft; a.hop = hop; a.n_mels = n_mels;
    a.amin = amin; a.top_db = top_db; a.pad_mode = pad_mode; a.spf = frames_per_slice;
    a.db_floor = (float)(20.0 * std::log10((double)amin));   // exact value for clamped bins
    a.twiddle = c->spec.twiddle; a.window = c->spec.window;
    a.mel_start = c->spec.mel.start; a.mel_width = c->spec.mel.width; a.mel_weight = c->spec.mel.weight;
    a.mel_max_width = c->spec.mel.max_width;
    std::memcpy(a.mel_seg_nq, c->spec.mel.seg_nq, sizeof(a.mel_seg_nq));
    std::memcpy(a.mel_seg_nq4, c->spec.mel.seg_nq4, sizeof(a.mel_seg_nq4));
    a.umax = c->umax;
    *out = a;
    return 0;
}

// avse_istft's and its ragged form's parameter checks, in the order the C-ABI reports them.  n_frames: the uniform
// form's (with stft_frames); NULL for the ragged form, whose frame counts its RaggedGeom checks per utterance.
int istft_check(bool pointers, int64_t n_utt, const int* n_frames, int stft_frames, int frames_per_slice, int sr, int n_fft,
                int hop, int n_mels) {
    if (!pointers) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n_utt < 0 || (n_frames && (*n_frames < 1 || stft_frames < *n_frames)) || hop <= 0 || sr <= 0 || n_fft < 2)
        return fail(AVSE_ERR_INVALID, n_frames ? "bad istft geometry (need 1 <= n_frames <= stft_frames)" : "bad istft geometry");
    if (n_fft > 2048) return fail(AVSE_ERR_UNSUPPORTED, "n_fft > 2048 not supported");
    if (n_mels < 1 || n_mels > 80) return fail(AVSE_ERR_UNSUPPORTED, "n_mels must be in [1, 80]");
    if (frames_per_slice < 0 || (n_frames && frames_per_slice > 0 && *n_frames % frames_per_slice))
        return fail(AVSE_ERR_INVALID, n_frames ? "n_frames must be a multiple of frames_per_slice" : "frames_per_slice < 0");
    return 0;
}

// The tables of a checked ISTFT call and its launch arguments but for the frame counts (T, stft_frames, n_slices stay
// 0: the uniform form sets them; per utterance in a ragged batch) and the unfused kernels' frame scratch, which the
// caller grows (a.frames).
int istft_args(avse_ctx* c, const float* mel_db, const float* stft_ri, int64_t n_utt, int frames_per_slice, int sr,
               int n_fft, int hop, int n_mels, float fmin, float fmax, float* sig, IstftArgs* out) {
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = ensure_istft_tables(c, sr, n_fft, n_mels, fmin, fmax)) return rc;
    IstftArgs a;
    std::memset(&a, 0, sizeof(a));
    a.mel_db = mel_db; a.stft = reinterpret_cast<const float2*>(stft_ri); a.sig = sig;
    a.n_utt = n_utt; a.spf = frames_per_slice; a.hop = hop; a.n_mels = n_mels;
    a.nb = 1 + n_fft / 2; a.N = 2 * (a.nb - 1);
    a.pinvT = c->istft.pinvT; a.twiddle = c->istft.twiddle; a.window = c->istft.window;
    a.bins = c->istft.bins;
    a.gram_inv = c->opt.dense_istft ? nullptr : c->istft.gram_inv.p.get();
    *out = a;
    return 0;
}

// avse_eval_pairs_sized (flags 0, 5 slots per row) and avse_eval_pairs_ext (6 slots): one set of checks, one launch
int eval_pairs_call(avse_ctx* c, const float* ref, const float* deg, const int64_t* off, int64_t n_pairs,
                    int64_t total_samples, int sr, int flags, int slots, double* metrics, void* stream) {
    if (!c || !ref || !deg || !off || !metrics) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (flags & ~AVSE_EVAL_ANY_RATE) return fail(AVSE_ERR_INVALID, "unknown avse_eval_flags bit");
    if (n_pairs < 1) return fail(AVSE_ERR_INVALID, "bad eval_pairs shape (n_pairs >= 1)");
    if (sr < 8000 || sr > 48000) return fail(AVSE_ERR_INVALID, "sample rate outside 8000 .. 48000");
    if (n_pairs >= (1LL << 31)) return fail(AVSE_ERR_UNSUPPORTED, "n_pairs must be below 2^31");
    if (total_samples < 0 || total_samples > n_pairs * (1LL << 24))
        return fail(AVSE_ERR_INVALID, "total_samples outside 0 .. n_pairs * 2^24");
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    // The pair lengths live on the device and the call does not wait for them.  The scratch is sized for
    // total_samples, the caller's off[n_pairs] - off[0]; without it (0), for the most samples the two buffers can hold
    // behind ref / deg (the extent of their allocations).  The kernels treat offsets that pass the bound as empty pairs.
    int64_t cap = total_samples > 0 ? total_samples : n_pairs * (1LL << 24);
    for (const float* p : {ref, deg}) {
        if (total_samples > 0) break;
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
            (void)hipGetLastError();
            return fail(AVSE_ERR_INVALID, "ref / deg must point into device allocations (hipMalloc)");
        }
        const int64_t room = (int64_t)(((const char*)base + size) - (const char*)p) / (int64_t)sizeof(float);
        cap = std::min(cap, room);
    }
    if (cap < 1) return fail(AVSE_ERR_INVALID, "ref / deg hold no samples");
    const EvalTables* tables = nullptr;
    if (int rc = ensure_eval_tables(c, sr, (flags & AVSE_EVAL_ANY_RATE) != 0, (hipStream_t)stream, &tables)) return rc;
    const EvalTables& t = *tables;
    // the large ratios scale sample offsets by up to 10000 (eval.hip pair_geom, eval_layout): a cap whose product
    // would leave int64 could not be allocated anyway (25 bytes of scratch per sample)
    if (t.big && cap > (1LL << 40)) return fail(AVSE_ERR_OOM, "eval_pairs scratch for more than 2^40 samples");
    EvalDev d;
    d.taps = t.taps; d.W = t.W; d.twid = t.twid; d.segw = t.segw; d.bands = t.bands;
    d.ptaps = t.big ? t.ptaps.p.get() : nullptr;
    d.up = t.up; d.down = t.down; d.H = t.H;
    d.win = t.win; d.skip = t.win / 4;
    d.stoi = t.big || std::max(t.up, t.down) <= kEvalMaxRatio;
    d.cap = cap;
    d.ms = slots;
    if (int rc = grow(c->prep, eval_pairs_scratch_bytes(n_pairs, d), (hipStream_t)stream, "preprocess scratch")) return rc;
    return launch_eval_pairs(ref, deg, off, n_pairs, d, metrics, c->prep, (hipStream_t)stream);
}

}  // namespace

namespace avse {
// the STFT / mel tables of one geometry into `t` (kept when `t` already holds them); the current device's
int build_spec_tables(SpecTables& t, int sr, int n_fft, int n_mels, double fmin, double fmax) {
    if (t.sr == sr && t.n_fft == n_fft && t.n_mels == n_mels && t.fmin == fmin && t.fmax == fmax) return 0;
    t = SpecTables();
    const DftTables dft = dft_tables(n_fft);
    const MelBands mb = mel_bands(sr, n_fft, n_mels, fmin, fmax);
    if (int rc = table_to_device(dft.twiddle, t.twiddle)) return rc;
    if (int rc = table_to_device(dft.window, t.window)) return rc;
    if (int rc = table_to_device(mb.start, t.mel.start)) return rc;
    if (int rc = table_to_device(mb.width, t.mel.width)) return rc;
    if (int rc = table_to_device(mb.weight, t.mel.weight)) return rc;
    t.sr = sr; t.n_fft = n_fft; t.n_mels = n_mels; t.fmin = fmin; t.fmax = fmax;
    std::memcpy(t.mel.seg_nq, mb.seg_nq, sizeof(t.mel.seg_nq));
    std::memcpy(t.mel.seg_nq4, mb.seg_nq4, sizeof(t.mel.seg_nq4));
    t.mel.max_width = mb.max_width;
    return 0;
}

// pinv(mel), the inverse-DFT tables and, where the bank allows it, the fused kernel's tridiagonal form (spec_tables.cpp)
int build_istft_tables(IstftTables& t, int sr, int n_fft, int n_mels, double fmin, double fmax) {
    if (t.sr == sr && t.n_fft == n_fft && t.n_mels == n_mels && t.fmin == fmin && t.fmax == fmax) return 0;
    t = IstftTables();
    const IstftHostTables h = istft_tables(sr, n_fft, n_mels, fmin, fmax);
    const DftTables dft = dft_tables(2 * (n_fft / 2));
    if (int rc = table_to_device(h.pinvT, t.pinvT)) return rc;
    if (int rc = table_to_device(dft.twiddle, t.twiddle)) return rc;
    if (int rc = table_to_device(dft.window, t.window)) return rc;
    if (!h.bins.empty())
        if (int rc = table_to_device(h.bins, t.bins)) return rc;
    if (!h.gram_inv.empty())
        if (int rc = table_to_device(h.gram_inv, t.gram_inv)) return rc;
    t.sr = sr; t.n_fft = n_fft; t.n_mels = n_mels; t.fmin = fmin; t.fmax = fmax;
    return 0;
}

// checked build: wait for the stream, then report the first device-side check that fired (avse_common.h DebugHit)
int debug_poll(void* stream) {
    if constexpr (!kDebugBuild) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    AVSE_HIP_CHECK(hipStreamIsCapturing((hipStream_t)stream, &cs));
    if (cs != hipStreamCaptureStatusNone) return 0;   // no synchronisation inside a capture: checked on a later call
    AVSE_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    static const struct {
        int (*read)(DebugHit*);
        const char* what;
    } readers[] = {{debug_read_v1r, "k_conv_v1r"}, {debug_read_stft, "STFT"}, {debug_read_istft, "ISTFT"}};
    for (const auto& r : readers) {
        DebugHit h{};
        if (r.read(&h)) return fail(AVSE_ERR_HIP, "checked build: reading the device check record failed");
        if (h.hit)
            return fail(AVSE_ERR_CHECK, std::string("checked build: ") + r.what + " check " + std::to_string(h.code) +
                                            " failed (kernel id " + std::to_string(h.kernel) + ", block " +
                                            std::to_string(h.block) + ", thread " + std::to_string(h.thread) +
                                            ": value " + std::to_string(h.value) + ", expected " +
                                            std::to_string(h.expect) + ")");
    }
    return 0;
}
}  // namespace avse

avse_ctx::~avse_ctx() {
    (void)hipSetDevice(device);
    if (ragged_done) (void)hipEventDestroy(ragged_done);
    for (auto& g : graphs) (void)hipGraphExecDestroy(g.exec);
    if (cap) (void)hipStreamDestroy(cap);
    if (side) (void)hipStreamDestroy(side);
    if (fork) (void)hipEventDestroy(fork);
    if (join) (void)hipEventDestroy(join);
    for (hipEvent_t e : map_ev)
        if (e) (void)hipEventDestroy(e);
}   // then the members: every table and scratch buffer

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

int avse_abi_version(void) { return AVSE_ABI_VERSION; }

int avse_build_flags(void) { return avse::kDebugBuild ? 1 : 0; }
const char* avse_last_error(void) { return g_err.c_str(); }

int avse_ctx_create(int device, avse_ctx** out) {
    if (!out) return fail(AVSE_ERR_INVALID, "out is NULL");
    int n = 0;
    AVSE_HIP_CHECK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(AVSE_ERR_INVALID, "bad device index");
    AVSE_HIP_CHECK(hipSetDevice(device));
    avse_ctx* c = new avse_ctx();
    c->device = device;
    for (const OptionName& o : kOptionNames) {
        const char* e = std::getenv(o.env);
        if (e && *e) c->opt.*(o.field) = std::atoi(e);
    }
    if (c->mse_partial.alloc(sizeof(float) * 256) != hipSuccess ||
        c->gemm_counters.alloc(sizeof(int) * kGemmCounters) != hipSuccess ||
        hipMemset(c->gemm_counters, 0, sizeof(int) * kGemmCounters) != hipSuccess ||
        c->range.alloc(sizeof(unsigned) * 4) != hipSuccess ||
        hipMemset(c->range, 0, sizeof(unsigned) * 4) != hipSuccess ||
        c->range_host.alloc(sizeof(unsigned) * 4) != hipSuccess) {
        delete c;
        return fail(AVSE_ERR_OOM, "hipMalloc failed (ctx)");
    }
    *out = c;
    return 0;
}

void avse_ctx_destroy(avse_ctx* c) { delete c; }

int avse_ctx_set_option(avse_ctx* c, const char* name, int value) {
    if (!c || !name) return fail(AVSE_ERR_INVALID, "NULL argument");
    const OptionName* o = find_option(name);
    if (!o) return fail(AVSE_ERR_INVALID, std::string("unknown option '") + name + "'");
    c->opt.*(o->field) = value;
    return 0;
}

int avse_ctx_get_option(avse_ctx* c, const char* name, int* value) {
    if (!c || !name || !value) return fail(AVSE_ERR_INVALID, "NULL argument");
    const OptionName* o = find_option(name);
    if (!o) return fail(AVSE_ERR_INVALID, std::string("unknown option '") + name + "'");
    *value = c->opt.*(o->field);
    return 0;
}

int avse_spectrogram(avse_ctx* c, const float* sig, int64_t n_utt, int64_t n_samples, int sr, int n_fft, int hop,
                     int n_mels, float fmin, float fmax, float amin, float top_db, int pad_mode, int frames_per_slice,
                     float* mel_db, float* stft_ri, void* stream) {
    if (int rc = spec_check(c && sig && mel_db, n_utt, &n_samples, sr, n_fft, hop, n_mels, pad_mode, frames_per_slice))
        return rc;
    SpecArgs a;
    if (int rc = spec_args(c, sig, n_utt, sr, n_fft, hop, n_mels, fmin, fmax, amin, top_db, pad_mode, frames_per_slice,
                           mel_db, stft_ri, (hipStream_t)stream, &a))
        return rc;
    a.n_samples = n_samples;
    a.n_frames = (int)(1 + (n_samples + 2 * (n_fft / 2) - n_fft) / hop);   // centred frames (librosa.stft)
    a.n_slices = frames_per_slice > 0 ? a.n_frames / frames_per_slice : 0;
    if (int lr = launch_spectrogram(a, (hipStream_t)stream)) return lr;
    return debug_poll(stream);
}

int avse_istft(avse_ctx* c, const float* mel_db, const float* stft_ri, int64_t n_utt, int n_frames, int stft_frames,
               int frames_per_slice, int sr, int n_fft, int hop, int n_mels, float fmin, float fmax, float* sig,
               void* stream) {
    if (int rc = istft_check(c && mel_db && stft_ri && sig, n_utt, &n_frames, stft_frames, frames_per_slice, sr, n_fft, hop,
                             n_mels))
        return rc;
    if (n_utt == 0) return 0;
    IstftArgs a;
    if (int rc = istft_args(c, mel_db, stft_ri, n_utt, frames_per_slice, sr, n_fft, hop, n_mels, fmin, fmax, sig, &a))
        return rc;
    if (int rc = grow(c->frames, sizeof(float) * (size_t)n_utt * n_frames * a.N, (hipStream_t)stream, "istft scratch")) return rc;
    a.frames = c->frames;
    a.T = n_frames;
    a.stft_frames = stft_frames;
    a.n_slices = frames_per_slice > 0 ? n_frames / frames_per_slice : 0;
    if (int lr = launch_istft(a, (hipStream_t)stream)) return lr;
    return debug_poll(stream);
}

int avse_spectrogram_ragged(avse_ctx* c, const float* sig, const int64_t* sig_off, const int64_t* n_samples,
                            int64_t n_utt, int sr, int n_fft, int hop, int n_mels, float fmin, float fmax, float amin,
                            float top_db, int pad_mode, int frames_per_slice, float* mel_db, float* stft_ri,
                            void* stream) {
    if (int rc = spec_check(c && sig && sig_off && n_samples && mel_db, n_utt, nullptr, sr, n_fft, hop, n_mels, pad_mode,
                            frames_per_slice))
        return rc;
    if (n_utt > INT32_MAX) return fail(AVSE_ERR_INVALID, ragged_message(RAGGED_TOO_LARGE));
    // chunk: that of the kernel this n_fft runs in (the band table's width, known only with the tables, can still send
    // n_fft 533 to the run dispatch: the item table is then not used)
    const int chunk = spectrogram_ragged_chunk(n_fft, hop, n_mels, 0);
    const RaggedGeom g = ragged_spec_geom(sig_off, n_samples, n_utt, n_fft, hop, frames_per_slice, n_mels,
                                          pad_mode == AVSE_PAD_REFLECT, chunk > 0 ? chunk : 1 << 30);
    if (g.status != RAGGED_OK)
        return fail(AVSE_ERR_INVALID, std::string(ragged_message(g.status)) + " (utterance " + std::to_string(g.bad_utt) + ")");
    if (n_utt == 0) return 0;
    SpecArgs a;
    if (int rc = spec_args(c, sig, n_utt, sr, n_fft, hop, n_mels, fmin, fmax, amin, top_db, pad_mode, frames_per_slice,
                           mel_db, stft_ri, (hipStream_t)stream, &a))
        return rc;
    RaggedDev d = {nullptr, nullptr, 0, 0};
    if (g.runs.size() > 1 && spectrogram_ragged_chunk(n_fft, hop, n_mels, a.mel_max_width) > 0)
        if (int ur = upload_ragged(c, g, (hipStream_t)stream, &d)) return ur;
    if (int lr = launch_spectrogram_ragged(a, g, d, (hipStream_t)stream)) return lr;
    return debug_poll(stream);
}

int avse_istft_ragged(avse_ctx* c, const float* mel_db, const float* stft_ri, const int64_t* n_frames,
                      const int64_t* stft_frames, int64_t n_utt, int frames_per_slice, int sr, int n_fft, int hop,
                      int n_mels, float fmin, float fmax, float* sig, void* stream) {
    if (int rc = istft_check(c && mel_db && stft_ri && n_frames && stft_frames && sig, n_utt, nullptr, 0, frames_per_slice,
                             sr, n_fft, hop, n_mels))
        return rc;
    if (n_utt > INT32_MAX) return fail(AVSE_ERR_INVALID, ragged_message(RAGGED_TOO_LARGE));
    const int nb = 1 + n_fft / 2, N = 2 * (nb - 1);
    // chunk: the fused kernel's where the shape can run in it (without its tables the run dispatch serves, and the
    // item table is not used)
    const int chunk = istft_ragged_chunk(N, hop, n_mels, true);
    const RaggedGeom g = ragged_istft_geom(n_frames, stft_frames, n_utt, frames_per_slice, nb, hop, n_mels,
                                           chunk > 0 ? chunk : 1 << 30);
    if (g.status != RAGGED_OK)
        return fail(AVSE_ERR_INVALID, std::string(ragged_message(g.status)) + " (utterance " + std::to_string(g.bad_utt) + ")");
    if (n_utt == 0) return 0;
    IstftArgs a;
    if (int rc = istft_args(c, mel_db, stft_ri, n_utt, frames_per_slice, sr, n_fft, hop, n_mels, fmin, fmax, sig, &a))
        return rc;
    const bool in_kernel = g.runs.size() > 1 && istft_ragged_chunk(N, hop, n_mels, a.gram_inv && a.bins) > 0;
    size_t need = 0;   // the unfused kernels' frame scratch, for the largest run
    for (const RaggedRun& r : g.runs) need = std::max(need, sizeof(float) * (size_t)r.count * (size_t)g.utt[r.first].T * N);
    if (int rc = grow(c->frames, in_kernel ? 0 : need, (hipStream_t)stream, "istft scratch")) return rc;
    a.frames = c->frames;
    RaggedDev d = {nullptr, nullptr, 0, 0};
    if (in_kernel && !g.items.empty())
        if (int ur = upload_ragged(c, g, (hipStream_t)stream, &d)) return ur;
    if (int lr = launch_istft_ragged(a, g, d, (hipStream_t)stream)) return lr;
    return debug_poll(stream);
}

int avse_video_normalize(avse_ctx* c, float* video, int64_t S, int H, int W, int F, const float* mean,
                         const float* stdv, void* stream) {
    if (!c || !video || !mean || !stdv) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (S < 0 || H <= 0 || W <= 0 || F <= 0) return fail(AVSE_ERR_INVALID, "bad video shape");
    if (S == 0) return 0;
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    return launch_video_normalize(video, S, H, W, F, mean, stdv, (hipStream_t)stream);
}

int avse_mse(avse_ctx* c, const float* pred, const float* target, int64_t n, float* loss, void* stream) {
    if (!c || !pred || !target || !loss) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n <= 0) return fail(AVSE_ERR_INVALID, "n must be positive");
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    return launch_mse(pred, target, n, loss, c->mse_partial, (hipStream_t)stream);
}

int avse_mix_pairs(avse_ctx* c, const int16_t* speech, const int64_t* speech_off, const int16_t* noise,
                   const int64_t* noise_off, const double* snr_lin, int64_t n_pairs, int64_t L, float* rows,
                   double* mix64, double* factor, void* stream) {
    if (!c || !speech || !speech_off || !noise || !noise_off || !rows) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (n_pairs < 0 || L <= 0) return fail(AVSE_ERR_INVALID, "bad mix_pairs shape (n_pairs >= 0, L > 0)");
    if (L >= (1LL << 31)) return fail(AVSE_ERR_UNSUPPORTED, "L must be below 2^31 samples");
    if (n_pairs == 0) return 0;
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = grow(c->prep, mix_pairs_scratch_bytes(n_pairs), (hipStream_t)stream, "preprocess scratch")) return rc;
    return launch_mix_pairs(speech, speech_off, noise, noise_off, snr_lin, n_pairs, L, rows, mix64, factor, c->prep,
                            (hipStream_t)stream);
}

int avse_eval_pairs(avse_ctx* c, const float* ref, const float* deg, const int64_t* off, int64_t n_pairs, int sr,
                    double* metrics, void* stream) {
    return avse_eval_pairs_sized(c, ref, deg, off, n_pairs, 0, sr, metrics, stream);
}

int avse_eval_pairs_sized(avse_ctx* c, const float* ref, const float* deg, const int64_t* off, int64_t n_pairs,
                          int64_t total_samples, int sr, double* metrics, void* stream) {
    return eval_pairs_call(c, ref, deg, off, n_pairs, total_samples, sr, 0, AVSE_EVAL_NMETRICS, metrics, stream);
}

int avse_eval_pairs_ext(avse_ctx* c, const float* ref, const float* deg, const int64_t* off, int64_t n_pairs,
                        int64_t total_samples, int sr, int flags, double* metrics, void* stream) {
    return eval_pairs_call(c, ref, deg, off, n_pairs, total_samples, sr, flags, AVSE_EVAL_NMETRICS_EXT, metrics, stream);
}

int avse_video_stats(avse_ctx* c, const float* video, int64_t S, int H, int W, int F, float* mean, float* stdv,
                     void* stream) {
    return avse_video_stats_video(c, video, AVSE_VIDEO_F32, S, H, W, F, mean, stdv, stream);
}

int avse_video_stats_video(avse_ctx* c, const void* video, int vdt, int64_t S, int H, int W, int F, float* mean,
                           float* stdv, void* stream) {
    if (!c || !video || !mean || !stdv) return fail(AVSE_ERR_INVALID, "NULL argument");
    if (vdt != AVSE_VIDEO_F32 && vdt != AVSE_VIDEO_U8) return fail(AVSE_ERR_INVALID, "unknown video dtype");
    if (vdt == AVSE_VIDEO_U8 && ((uintptr_t)video & 3))
        return fail(AVSE_ERR_INVALID, "uint8 video must be 4-byte aligned (alignment of the base pointer)");
    if (S <= 0 || H <= 0 || W <= 0 || F <= 0) return fail(AVSE_ERR_INVALID, "bad video shape (every extent positive)");
    if (F > kVideoStatsMaxF) return fail(AVSE_ERR_UNSUPPORTED, "more than 8 frames per slice not supported");
    if ((int64_t)H * W * F >= (1LL << 31)) return fail(AVSE_ERR_UNSUPPORTED, "H * W * F must be below 2^31");
    AVSE_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = grow(c->prep, video_stats_scratch_bytes(S, H, W), (hipStream_t)stream, "preprocess scratch")) return rc;
    if (vdt == AVSE_VIDEO_U8)
        return launch_video_stats_u8(reinterpret_cast<const uint8_t*>(video), S, H, W, F, mean, stdv, c->prep,
                                     (hipStream_t)stream);
    return launch_video_stats(reinterpret_cast<const float*>(video), S, H, W, F, mean, stdv, c->prep,
                              (hipStream_t)stream);
}

}  // extern "C"
