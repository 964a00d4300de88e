// Host-only layer geometry (no HIP header): the phase / tap tables every layer of the plan (netplan.h) runs with on
// k_conv, for the inference forward (forward.hip), the training forward and its input gradient (train.hip), and the
// index maps from the Keras kernel to the packed [phase][rows][kpad] weights (weight_pack.cpp, train.hip).
#pragma once
#include <utility>
#include <vector>

#include "netplan.h"

namespace avse {

constexpr int MAX_TAPS = 25;
constexpr int MAX_PHASES = 4;

struct ConvPhase {
    int py, px;          // output phase offset (deconv); 0 for forward convs
    int ntaps;
    int kpad;            // ntaps * cin padded to the k-slab (multiple of 32)
    long long w_off;     // element offset of this phase's packed weights [cout][kpad]
    int tap_off;         // offset of this phase's (dy, dx) pairs in ConvArgs::taps
};

struct Tap {   // input offset of one tap: the layout of HIP's int2 (x = dy, y = dx; asserted where it is uploaded)
    int dy, dx;
};

// Keras kernel element index for (ky, kx, in-channel ci, out-channel co) of layer L
inline long long kidx(const LayerDef& L, int ky, int kx, int ci, int co) {
    if (L.kind == DENSE) return (long long)ci * L.cout + co;
    if (L.kind == CONV) return (((long long)ky * L.kw + kx) * L.cin + ci) * L.cout + co;
    return (((long long)ky * L.kw + kx) * L.cout + co) * L.cin + ci;   // transposed conv (kh, kw, cout, cin)
}

// One axis of a phase: the kernel taps k it uses and the grid offset each reads at.
struct AxisTap {
    int k, off;
};
typedef std::vector<std::vector<AxisTap>> AxisPhases;

// Sub-pixel decomposition of a stride-s scatter y[q s + k - pad] += x[q] w[k] into s gathers: phase r = output index
// mod s takes the taps k with (r + pad - k) % s == 0 and reads x at q + (r + pad - k) / s.  The forward of a
// transposed convolution and the input gradient of a strided convolution are both this.
inline AxisPhases subpixel_phases(int k, int s, int pad) {
    AxisPhases ph(s);
    for (int r = 0; r < s; ++r)
        for (int kk = 0; kk < k; ++kk) {
            const int d = r + pad - kk;
            if (((d % s) + s) % s == 0) ph[r].push_back({kk, d / s});
        }
    return ph;
}

// The single phase of a gather y[q] = sum_k x[q s + k - pad] w[k]: every tap k, at offset k - pad.
inline AxisPhases gather_taps(int k, int pad) {
    AxisPhases ph(1);
    for (int kk = 0; kk < k; ++kk) ph[0].push_back({kk, kk - pad});
    return ph;
}

enum GeomStatus { GEOM_OK = 0, GEOM_TOO_MANY_PHASES, GEOM_DGRAD_STRIDE, GEOM_DGRAD_EMPTY_PHASE };
inline const char* geom_message(GeomStatus s) {
    switch (s) {
        case GEOM_TOO_MANY_PHASES: return "deconv stride too large";
        case GEOM_DGRAD_STRIDE: return "conv dgrad needs input dims divisible by the stride";
        case GEOM_DGRAD_EMPTY_PHASE: return "conv dgrad phase without taps";
        default: return "";
    }
}

// The phases of one gather convolution on k_conv: per phase [rows][kpad] weights, k = tap * cp + channel.
struct PhaseSet {
    GeomStatus status = GEOM_OK;
    bool dgrad = false;   // rows are the layer's input channels and the reduction runs over its output channels
    int rows = 0, red = 0, cp = 0;   // packed rows, reduction channels and their stride (red padded to 8)
    int nphase = 0;
    ConvPhase ph[MAX_PHASES] = {};
    std::vector<Tap> taps;                                 // all phases (ConvPhase::tap_off)
    std::vector<std::vector<std::pair<int, int>>> kyx;     // per phase, the Keras (ky, kx) of each tap
    long long w_elems = 0;                                 // size of the packed weights
};

// phase (py, px) = Y[py] x X[px], ky outermost; kpad = taps x cp rounded up to 32
inline void set_phases(PhaseSet& g, const AxisPhases& Y, const AxisPhases& X) {
    if (Y.size() * X.size() > (size_t)MAX_PHASES) {
        g.status = GEOM_TOO_MANY_PHASES;
        return;
    }
    for (int py = 0; py < (int)Y.size(); ++py)
        for (int px = 0; px < (int)X.size(); ++px) {
            const int ntaps = (int)(Y[py].size() * X[px].size());
            const int kpad = (int)(((long long)ntaps * g.cp + 31) / 32 * 32);
            g.ph[g.nphase++] = ConvPhase{py, px, ntaps, kpad, g.w_elems, (int)g.taps.size()};
            g.kyx.emplace_back();
            for (const AxisTap& y : Y[py])
                for (const AxisTap& x : X[px]) {
                    g.kyx.back().push_back({y.k, x.k});
                    g.taps.push_back(Tap{y.off, x.off});
                }
            g.w_elems += (long long)g.rows * kpad;
        }
}

inline int pad8(int c) { return (c + 7) / 8 * 8; }

// Forward geometry.  CONV: TF 'SAME'; DENSE is the 1 x 1 case of it; DECONV: TF conv2d_transpose 'SAME' to in * s,
// cropped at pad_before = max(k - s, 0) / 2, as one gather per output phase.
struct LayerGeom : PhaseSet {
    int cin_pad = 0;       // channel stride of the input (a 16-B chunk never straddles a tap)
    int pt = 0, pl = 0;    // padding before (rows, columns)
    int hq = 1, wq = 1;    // the grid k_conv walks per phase
    int hz = 1, wz = 1;    // the layer's output before pooling (DECONV: hq x wq times the stride)
    int ho = 1, wo = 1;    // after the 2 x 2 max pool
};

inline LayerGeom layer_geom(const LayerDef& L) {
    LayerGeom g;
    g.cin_pad = g.cp = pad8(L.cin);
    g.rows = L.cout;
    g.red = L.cin;
    if (L.kind == DECONV) {
        g.pt = (L.kh > L.sh ? L.kh - L.sh : 0) / 2;
        g.pl = (L.kw > L.sw ? L.kw - L.sw : 0) / 2;
        g.hq = L.hin;
        g.wq = L.win;
        g.hz = L.hin * L.sh;
        g.wz = L.win * L.sw;
        set_phases(g, subpixel_phases(L.kh, L.sh, g.pt), subpixel_phases(L.kw, L.sw, g.pl));
    } else {
        g.pt = same_pad_before(L.hin, L.kh, L.sh);
        g.pl = same_pad_before(L.win, L.kw, L.sw);
        g.hq = g.hz = same_out(L.hin, L.sh);
        g.wq = g.wz = same_out(L.win, L.sw);
        set_phases(g, gather_taps(L.kh, g.pt), gather_taps(L.kw, g.pl));
    }
    g.ho = L.pool ? g.hz / 2 : g.hz;
    g.wo = L.pool ? g.wz / 2 : g.wz;
    return g;
}

// Input-gradient geometry: dL/dx as a gather over dz (the layer's pre-pool output gradient, channel stride ci).
// CONV (DENSE: its 1 x 1 case): dx[q s + r] per phase r, taps ky = r + pt (mod s) at dz row q + (r + pt - ky) / s.
// DECONV: din[iy] = sum_ky dout[iy s + ky - pt] W[ky], a strided conv of dout.
struct DgradGeom : PhaseSet {
    int ci = 0;              // dz channel stride (d_deconv6: 8)
    int hq = 1, wq = 1;      // grid per phase
    int sy = 1, sx = 1;      // dz step per grid step
    int oys = 1, oxs = 1;    // dx step per grid step
};

inline DgradGeom dgrad_geom(const LayerDef& L) {
    const LayerGeom f = layer_geom(L);
    DgradGeom g;
    g.dgrad = true;
    g.ci = g.cp = pad8(L.cout);
    g.rows = L.cin;
    g.red = L.cout;
    if (L.kind == DECONV) {
        g.hq = L.hin;
        g.wq = L.win;
        g.sy = L.sh;
        g.sx = L.sw;
        set_phases(g, gather_taps(L.kh, f.pt), gather_taps(L.kw, f.pl));
        return g;
    }
    if (L.hin % L.sh || L.win % L.sw) {
        g.status = GEOM_DGRAD_STRIDE;
        return g;
    }
    g.hq = L.hin / L.sh;
    g.wq = L.win / L.sw;
    g.oys = L.sh;
    g.oxs = L.sw;
    set_phases(g, subpixel_phases(L.kh, L.sh, f.pt), subpixel_phases(L.kw, L.sw, f.pl));
    for (int p = 0; p < g.nphase && g.status == GEOM_OK; ++p)
        if (g.ph[p].ntaps == 0) g.status = GEOM_DGRAD_EMPTY_PHASE;
    return g;
}

// [phase][row][kpad] -> Keras kernel element of layer L, -1 for padding
inline std::vector<int> gather_map(const LayerDef& L, const PhaseSet& g) {
    std::vector<int> m((size_t)g.w_elems, -1);
    for (int p = 0; p < g.nphase; ++p)
        for (int n = 0; n < g.rows; ++n) {
            int* row = m.data() + (size_t)g.ph[p].w_off + (size_t)n * g.ph[p].kpad;
            for (size_t j = 0; j < g.kyx[p].size(); ++j) {
                const int ky = g.kyx[p][j].first, kx = g.kyx[p][j].second;
                const long long k0 = g.dgrad ? kidx(L, ky, kx, n, 0) : kidx(L, ky, kx, 0, n);
                const long long dk = (g.dgrad ? kidx(L, ky, kx, n, 1) : kidx(L, ky, kx, 1, n)) - k0;   // per reduction channel
                for (int c = 0; c < g.red; ++c) row[j * g.cp + c] = (int)(k0 + c * dk);
            }
        }
    return m;
}

// k_conv's fp32 blocked summation: K-slabs (16 products each) summed FP32_BLOCK at a time into a zeroed partial that
// is added to the running sum in slab order.  A split-K whose every split is exactly one such block, reduced in split
// order, therefore reproduces the unsplit sums bit for bit (train.hip train_split).
constexpr int kFp32Block = 8;

// gemm.hip's split-K tickets: one int per 128 x 128 output tile of a launch, in a per-context array of kGemmCounters.
// A split launch (ksplit > 1) with more tiles than counters does not fit: launch_gemm declines it and the forward runs
// that layer on k_conv.  (The split dtype's dense layers always split: dec_dense2's 25 column tiles pass the array at
// 327 row tiles, about 41.9K clips.)
constexpr int kGemmCounters = 8192;
inline bool gemm_tickets_fit(long long M, long long N, int ksplit, long long counters) {
    return ksplit <= 1 || ((M + 127) / 128) * ((N + 127) / 128) <= counters;
}

}  // namespace avse
