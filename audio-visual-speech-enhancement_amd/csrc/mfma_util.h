// Device-side vocabulary of the matrix-core kernels (gfx950): the constants, buffer descriptors, LDS swizzles,
// barriers, MFMA wrappers, epilogue pieces and the split-pair encoding that conv*.hip, gemm.hip, train.hip, istft.hip,
// stft.hip and frame640.h share.  Everything here is __device__ __forceinline__ or constexpr: including it adds no code, and a
// kernel built on it compiles to the instructions of the same text written out (tools/isa_diff.py checks two builds).
#pragma once
#include <utility>

#include "avse_common.h"

namespace avse {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

// ---- constants ---------------------------------------------------------------------------
constexpr float LRELU = 0.3f;       // LeakyReLU slope of every layer (network.py)
// A buffer offset that reads as zero and stores nothing: past every resource make_rsrc builds, which is also why
// make_rsrc clamps num_records to it.  "Load or zero" is then a select of the offset, not a branch around the load
// (a branch makes hipcc drain vmcnt per load).
constexpr int kOOB = 0x7fffff00;

// ---- buffer descriptors ------------------------------------------------------------------
// Raw buffer resource over [base, base + bytes): bytes clamped to [0, kOOB]; a zero-sized resource reads zeros and
// drops stores (how a missing clip of a ragged grid is masked).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, long long bytes) {
    const int nrec = bytes > kOOB ? kOOB : (bytes < 0 ? 0 : (int)bytes);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, nrec, 0x00020000);
}
// The same without the lower clamp, for a size the caller knows is not negative: k_istft_fused, where the clamp at 0
// costs four scalar instructions per utterance that the kernel was measured without.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc_nonneg(const void* base, long long bytes) {
    const int nrec = bytes > kOOB ? kOOB : (int)bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, nrec, 0x00020000);
}

// ---- LDS access --------------------------------------------------------------------------
__device__ __forceinline__ i32x4 lds16(const char* base, int off) { return *reinterpret_cast<const i32x4*>(base + off); }
__device__ __forceinline__ void st16(char* p, i32x4 v) { *reinterpret_cast<i32x4*>(p) = v; }

// ---- swizzles and the slab image ---------------------------------------------------------
// A weight (or im2col) slab in LDS is rows of 64 B: four 16-B k-groups of one output channel (or pixel).  A
// ds_read_b128 of an MFMA operand takes one 16-B group per lane, and rows 64 B apart put every fourth row on the
// same banks, so group g of row r is stored in slot g ^ f(r):
//   wsw   conflict-free for the ds_read_b128 lane groups of the v_mfma_f32_16x16x32 operand (lane l: row l & 15,
//         k-group l >> 4), planar split reads (groups kg & 1 and 2 + (kg & 1)) included: every fused and tiled kernel's
//         weight ring, k_gemm's A and W slabs, k_conv_v1r's weight image.  Found by the exhaustive search of
//         tools/lds_swizzle_search.py ("weight swizzles"; --gemm and --tail re-check it for those kernels).
//   wswz  <true> is wsw; <false> is the same search's result for the v_mfma_f32_32x32x16 operand (lane l: row l & 31,
//         k-groups 2 m + (l >> 5)) of k_conv_stream's 32-row compute waves.
//   swz   the generic kernels' A and B slabs (k_conv, k_conv_win): the same 16x16x32 reads.  It predates the search
//         script, which does not cover it; a kernel that is not k_conv's slab loop wants wsw.
__device__ __forceinline__ int wsw(int row) { return 2 * ((row >> 2) & 1); }
template <bool M16> __device__ __forceinline__ int wswz(int row) { return M16 ? wsw(row) : (row >> 2) & 3; }
__device__ __forceinline__ int swz(int row) { return ((row >> 3) & 1) * 3; }
// byte address of k-group `kgroup` of row `row` in a wsw-swizzled slab of 64-B rows that starts at `base`.  The sum
// is taken in this order (base + row, then the slot): the compiler does not reassociate it, and another order moves
// registers in the kernels that were tuned with this one.
__device__ __forceinline__ int slab_row_addr(int row, int kgroup, int base = 0) {
    return base + row * 64 + ((kgroup ^ wsw(row)) << 4);
}
// the same address from the slot (kgroup ^ wsw(row)) the caller computed: k_dec_tail's and k_aud_enc's fragment base
// (bfr) need this form, slab_row_addr there swaps the operands of one v_bitop3_b32
__device__ __forceinline__ int slab_slot_addr(int row, int slot, int base = 0) { return base + row * 64 + (slot << 4); }

// ---- synchronisation ---------------------------------------------------------------------
// All as asm with a memory clobber: the compiler moves no memory access across them and, unlike __syncthreads(), adds
// no vmcnt(0) drain of global loads that are meant to stay in flight.
__device__ __forceinline__ void barrier_raw() { asm volatile("s_barrier" ::: "memory"); }
// this wave's LDS operations drained, then the workgroup barrier
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// the same as two asm statements: k_dec_tail_s16 needs this form (as one statement the compiler schedules the code
// around it differently and the kernel's instructions change)
__device__ __forceinline__ void lds_barrier_split() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
}
// wave-synchronous LDS hand-off: a wave's LDS operations complete in issue order, so draining lgkmcnt (and keeping the
// compiler from moving memory operations across) is enough when every lane that wrote belongs to the reading wave
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// s_waitcnt vmcnt(N) lgkmcnt(0): all but the N youngest global loads have landed, LDS drained
template <int N>
__device__ __forceinline__ void wait_vm_lgkm0() {
    static_assert(N >= 0 && N < 64, "vmcnt range");
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

// ---- compile-time helper -----------------------------------------------------------------
// f(integral_constant<int, I>{}) for every I of the sequence, in order: a slab schedule whose steps are constants
template <int... I, typename F>
__device__ __forceinline__ void unroll(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}

// ---- MFMA wrappers -----------------------------------------------------------------------
// v_mfma_f32_16x16x32_{bf16,f16} on operands held as the four dwords a ds_read_b128 / buffer load delivers
__device__ __forceinline__ f32x4 mfma_bf16(i32x4 a, i32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_f16(i32x4 a, i32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// ---- epilogue pieces ---------------------------------------------------------------------
// LeakyReLU(0.3) in three forms.  For finite x all three give the same bits (0.3 x < x exactly when x > 0); they are
// kept apart because they compile to different instructions, and every kernel keeps the form it was measured and
// verified with.  Do not merge them.
//   lrelu_vmax    one v_max_f32 through inline asm, so the compiler adds no canonicalising v_max/v_mul before it:
//                 k_dec_tail, k_dec_head, k_aud_enc (through bn_lrelu_vmax), k_conv_v1r's bf16 epilogue
//   lrelu_fmax    fmaxf(x, 0.3 x): k_dec_tail_s16 (through bn_lrelu_fmax), k_conv_stream, k_conv_v1r's split epilogues
//   lrelu_select  x >= 0 ? x : 0.3 x, after a separate multiply-add: k_conv, k_conv_win, k_gemm, k_aconv1_split; the
//                 training kernels (train.hip act_bn) write the same expression out, their backward pass tests its sign
// NaN: lrelu_vmax and lrelu_fmax return the non-NaN operand of the max, lrelu_select keeps a NaN; the split layers
// report a NaN through the range guard below before it matters.
__device__ __forceinline__ float lrelu_vmax(float x) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(LRELU * x));   // LeakyReLU, no canonicalise
    return r;
}
__device__ __forceinline__ float lrelu_fmax(float x) { return fmaxf(x, LRELU * x); }
__device__ __forceinline__ float lrelu_select(float x) { return x >= 0.f ? x : LRELU * x; }
// folded BatchNorm (one fma) + LeakyReLU
__device__ __forceinline__ float bn_lrelu_vmax(float acc, float sc, float sh) { return lrelu_vmax(fmaf(acc, sc, sh)); }
__device__ __forceinline__ float bn_lrelu_fmax(float acc, float sc, float sh) { return lrelu_fmax(fmaf(acc, sc, sh)); }
// four floats -> four bf16 (RNE, as (bf16_t) casts), a, b in the first dword
__device__ __forceinline__ i32x2 pack4_bf16(float a, float b, float c, float d) {
    const bf16x2 lo = __builtin_convertvector((f32x2){a, b}, bf16x2), hi = __builtin_convertvector((f32x2){c, d}, bf16x2);
    return (i32x2){__builtin_bit_cast(int, lo), __builtin_bit_cast(int, hi)};
}

// ---- split pairs (AVSE_F32_SPLIT, DESIGN.md §3 split-f16) --------------------------------
// An fp32 value x travels as two f16, h = f16(x) and l = f16(x - h).  In the pair layout a pixel's channels lie in runs
// of 16 as [h(16) | l(16)]: channel n has its h at half pair_slot(n) of the pixel and its l 16 halves further on.
struct SplitPair { _Float16 h, l; };
// the two halves one at a time, for the sites that must store h before l is computed (the statement order reaches
// the instruction scheduler: k_dec_tail_s16's d_deconv4 epilogue); everything else calls split_pair
__device__ __forceinline__ _Float16 pair_h(float x) { return (_Float16)x; }
__device__ __forceinline__ _Float16 pair_l(float x, _Float16 h) { return (_Float16)(x - (float)h); }
__device__ __forceinline__ SplitPair split_pair(float x) {
    const _Float16 h = pair_h(x);
    return {h, pair_l(x, h)};
}
constexpr int kPairL = 16;          // halves from a value's h to its l
// pair_slot(pixel, n): from the pixel's base (a pointer to halves, or an offset in halves), summed in this order
template <typename B>
__device__ __forceinline__ constexpr B pair_slot(B pixel, int n) { return pixel + 32 * (n >> 4) + (n & 15); }
__device__ __forceinline__ constexpr int pair_slot(int n) { return pair_slot(0, n); }
// Range guard: x cannot be carried as a pair when h would be infinite (|x| >= 65520, the f16 overflow threshold under
// round-to-nearest-even) or x is NaN.  Kernels fold the test over the values a lane stores and report once (one vector
// atomic from the lanes that saw one; the flag word is sticky until avse_range_status / avse_forward_checked read it).
__device__ __forceinline__ bool pair_out_of_range(float x) { return !(__builtin_fabsf(x) < 65520.f); }
__device__ __forceinline__ void range_report(unsigned* flag, unsigned bit, bool bad) {
    if (bad && flag) atomicOr(flag, bit);
}

}  // namespace avse
