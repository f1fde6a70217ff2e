// The epilogue as integer thresholds (qnn_abi.h, qnn_fold_prepare): device functions shared by the kernels that use a
// fold and by the prepare / verify / eval kernels of qnn_fold.hip -- ONE definition, so what the sweep proves is what
// the kernels execute.
//
// Per output channel the reference's chain  bias_add -> BatchNormalization -> [+ shortcut, * 0.5] -> quantized_tanh
// (models/vgg.py:16-17, models/resnet.py:59-63,127-129; float32, one rounding per operation) is a monotone step function
// of the integer accumulator.  Folded form, on the accumulator in matrix-pipe units accw = 256 * acc (both int4 operands
// are widened to code * 16) with the per-channel offset beta already added (it is the MFMA's initial accumulator):
//     u  = float(accw) * A                          v_cvt_f32_i32, v_mul_f32            (exact conversion: |accw| < 2^24)
//     T  = snorm16(u) = rint(clamp(u, -1, 1) * 32767)   v_cvt_pknorm_i16_f32, two values per instruction
//   no shortcut:   T is Q12 (code * 4096 + fraction), saturated to the 4-bit code range by the conversion itself;
//   shortcut sc:   T is Q11;  W = sat16(T + (sc + 8) * 1024);  T' = sat16(W + W)   two v_pk_add_i16 clamp per pair
//     code = T >> 12 (arithmetic): the top nibble of each 16-bit half IS the two's-complement code.
// Pairs of values live in the two halves of one register from the conversion on.
//
// Second form ("bits", mode 2; tried first by qnn_fold_prepare -- it needs the thresholds, not the whole domain, inside
// |accw + beta| < 2^22: beyond that the bit pattern leaves the constant's binade, which keeps the order and only saturates): the stored
// offset is beta + 0x4B400000, so the integer accumulator IS the bit pattern of the float 12582912 + (accw + beta), and
//     u = fma(as_float(acc), A, C),   C = float(-12582912 * A)                    one v_fma_f32, no conversion
// replaces the conversion and the multiply (the residue 12582912 * A + C is a constant the offset search absorbs).
#pragma once
#include "qnn_common.h"

#ifdef __HIPCC__
typedef short qnn_s2 __attribute__((ext_vector_type(2)));

constexpr int kFoldMagicBits = 0x4B400000;          // float bits of 12582912 = 1.5 * 2^23 (ulp 1)
constexpr double kFoldMagic = 12582912.0;

// two accumulators (offset included) -> two saturated Q12 (no shortcut) / Q11 (shortcut) values
__device__ __forceinline__ uint32_t qnn_fold_pair(int accw0, int accw1, float a0, float a1) {
    const float u0 = __fmul_rn((float)accw0, a0), u1 = __fmul_rn((float)accw1, a1);
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pknorm_i16(u0, u1));
}
// the same on accumulators that carry the magic constant ("bits" form)
__device__ __forceinline__ uint32_t qnn_fold_pair_bits(int acc0, int acc1, float a0, float a1, float c0, float c1) {
    const float u0 = __fmaf_rn(__int_as_float(acc0), a0, c0), u1 = __fmaf_rn(__int_as_float(acc1), a1, c1);
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pknorm_i16(u0, u1));
}
// Third form (mode 3): the typed image entry (QNN_STORE_U8 / QNN_STORE_F32_IMAGE first layers), whose accumulator is the
// exact integer S = sum byte * code in units of ONE (no widening).  The folded form takes its offset in the FMA,
// u = fma(float(S), A, C),  and the rounding add, the integer median and the shift-adds of the packing go
// (v_cvt_pknorm_i16_f32 + v_perm_b32 / v_bfi_b32 instead).  These are the constants the handle reports and evaluates.
// The sub-step offset the bits form needs exists here too: with the accumulator seeded with 0x4B400000 the FMA's
// constant C' = float(C - 12582912 A') has magnitude in the hundreds, so its ulp is a sizeable fraction of one step of
// S, and an integer beta (|beta| <= 127, one more product of the MFMA's offset K-block) moves the thresholds by whole
// steps: neighbouring C' and beta together place them anywhere.  qnn_fold_prepare searches (A', C', beta) behind the
// mode-3 search and proves them on the whole domain with qnn_fold_pair_bits; if every channel passes, the layer's
// operand table (below) carries them and the kernel drops the conversion.
__device__ __forceinline__ uint32_t qnn_fold_pair_fma(int s0, int s1, float a0, float a1, float c0, float c1) {
    const float u0 = __fmaf_rn((float)s0, a0, c0), u1 = __fmaf_rn((float)s1, a1, c1);
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pknorm_i16(u0, u1));
}
template <int MODE>
__device__ __forceinline__ uint32_t qnn_fold_pair_m(int acc0, int acc1, float a0, float a1, float c0, float c1) {
    if constexpr (MODE == 2) return qnn_fold_pair_bits(acc0, acc1, a0, a1, c0, c1);
    else return qnn_fold_pair(acc0, acc1, a0, a1);
}
// shortcut merge: s = ((sc + 8) << 10) in both halves (offset-coded shortcut codes at Q11 / 2)
__device__ __forceinline__ uint32_t qnn_fold_merge(uint32_t t, uint32_t s) {
    const qnn_s2 w = __builtin_elementwise_add_sat(__builtin_bit_cast(qnn_s2, t), __builtin_bit_cast(qnn_s2, s));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_add_sat(w, w));
}
// the 4-bit codes of a pair (tests / verifier; the kernels pick the nibbles up with v_perm_b32 / v_bfi_b32)
__device__ __forceinline__ int qnn_fold_code_lo(uint32_t t) { return (int)(short)(t & 0xFFFFu) >> 12; }
__device__ __forceinline__ int qnn_fold_code_hi(uint32_t t) { return (int)t >> 28; }
// one value: accw = accumulator + stored offset; mode 1 (conversion + multiply) or 2 (bits); sc ignored without a shortcut
__device__ __forceinline__ int qnn_fold_code(int accw, float a, float c, int mode, bool res, int sc) {
    uint32_t t = mode == 2 ? qnn_fold_pair_bits(accw, accw, a, a, c, c)
                 : mode == 3 ? qnn_fold_pair_fma(accw, accw, a, a, c, c) : qnn_fold_pair(accw, accw, a, a);
    if (res) t = qnn_fold_merge(t, (uint32_t)((sc + 8) << 10) * 0x00010001u);
    return qnn_fold_code_lo(t);
}

// ---- operands of the byte first layer (qnn_first_u8.hip), per (filter block nt, lane = 16 kq + r) -------------------
// B operand of MFMA column r, K-block kq (kq < 3: the nine taps x (3 channels + one zero byte) of tap row kq and four
// zero bytes; kq = 3: the offset block, against A bytes of -128) and the two constants of the map behind the sum.
// DEAL (pooled int4 forms): column r of block nt is channel 4 r + nt, and the filter of a channel with negative BN
// scale is negated, A with it (pooling is a max on the integers).  fa / fc: per-channel constants of a fold that
// replace the affine map, or nullptr.  fbeta (bits form only, with fa / fc): byte 15 of the offset block carries
// beta[c] -- it meets an A byte of +1 -- and the other fifteen bytes sum to -sum k.
// ONE definition: the kernel's own preamble and the table qnn_fold_prepare builds once per handle both call it, so the
// table holds, bit for bit, what a launch without it computes.  Every lane of the wave must call it (two shuffles).
struct FirstU8Entry {
    uint32_t wd[4];
    float A, B;
};
template <bool DEAL>
__device__ __forceinline__ FirstU8Entry qnn_first_u8_entry(const EpiArgs& e, const float* __restrict__ wq, float wscale,
                                                           float D, int nt, int lane, const float* __restrict__ fa,
                                                           const float* __restrict__ fc,
                                                           const int32_t* __restrict__ fbeta) {
    const int r = lane & 15, kq = lane >> 4;
    const int c = DEAL ? 4 * r + nt : nt * 16 + r;
    const float bias = e.bias ? e.bias[c] : 0.0f;
    const float inv = e.bn_inv ? e.bn_inv[c] : 1.0f;
    const float shift = e.bn_inv ? e.bn_shift[c] : 0.0f;
    const bool flip = DEAL && inv < 0.0f;                    // pool with max only: negate the filter and A[c]
    const float* wrow = wq + (size_t)c * 27 + (kq < 3 ? kq : 2) * 9;
    int part = 0;
    FirstU8Entry t;
    t.wd[0] = t.wd[1] = t.wd[2] = t.wd[3] = 0u;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        int code = (int)rintf(__fmul_rn(wrow[i], wscale));
        if (flip) code = -code;
        if (kq == 3) code = 0;
        part += code;
        t.wd[i / 3] |= (uint32_t)(code & 0xFF) << (8 * (i % 3));
    }
    part += __shfl_xor(part, 16);                            // sum of the 27 codes of filter c (all four K-block
    part += __shfl_xor(part, 32);                            // lanes end up with it)
    if (kq == 3) {
        // bytes that sum to -part: against A bytes of -128 they contribute +128 * sum k (sixteen, or fifteen and beta)
        int rem = -part;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            int b = min(max(rem, -127), 127);
            if (fbeta && j == 15) b = fbeta[c];
            else rem -= b;
            t.wd[j >> 2] |= (uint32_t)(b & 0xFF) << (8 * (j & 3));
        }
    }
    if (fa) {
        t.A = fa[c]; t.B = fc[c];
    } else {
        // the affine map behind S (qnn_abi.h): float64 from the float32 constants, one rounding each
        const double m = e.fn == QNN_FN_QUANTIZED_TANH ? (double)e.act_m : 1.0;
        t.A = (float)((double)inv * m / (double)D);
        t.B = (float)(((double)bias * (double)inv + (double)shift) * m);
    }
    if (flip) t.A = -t.A;
    return t;
}
// The table in device memory, in uint4 units: [nt][lane] the B operands, then [lane] {A of blocks 0..3}, then [lane]
// {B (the FMA's constant) of blocks 0..3}: six coalesced 16-byte loads per lane.
constexpr int kFirstTabVec = 6 * 64;
__device__ __forceinline__ void qnn_first_u8_tab_store(uint4* __restrict__ tab, int nt, int lane, const FirstU8Entry& t) {
    tab[nt * 64 + lane] = make_uint4(t.wd[0], t.wd[1], t.wd[2], t.wd[3]);
    reinterpret_cast<float*>(tab + 4 * 64 + lane)[nt] = t.A;
    reinterpret_cast<float*>(tab + 5 * 64 + lane)[nt] = t.B;
}

// ---- per-lane epilogue constants of k_conv_mfma_halo (qnn_mfma_areg.hip) with a "bits" fold ---------------------------
// Lane li of a wave owns the channels c = nbase + 32 b + li (b = 0, 1) of its 64-filter slice: slope and FMA constant of
// the fold, the accumulator offset in its int8 value (fold_b: the MFMA's initial accumulator) and in its FP6 value (added
// to the pooled bit pattern << 8:  - 2048 sum(w) - (0x4B400000 << 8) on top, modulo 2^32; 0 without wsum), and bit b of
// `neg` = the channel's BN scale is negative (its 2x2 window is pooled by the minimum).
// ONE definition: the kernel's own preamble (QNN_EPI_NO_HALO_TAB, or no table in the handle) and the table
// qnn_fold_prepare builds once per mode-2 handle both call it, so the table holds what a launch without it computes.
struct HaloEpiEntry {
    float a[2], c[2];
    int b8[2], b6[2];
    uint32_t neg;
};
__device__ __forceinline__ HaloEpiEntry qnn_halo_epi_entry(const EpiArgs& e, const int32_t* __restrict__ wsum, int nbase,
                                                           int li) {
    HaloEpiEntry t;
    t.neg = 0u;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int c = nbase + b * 32 + li;
        t.a[b] = e.fold_a[c]; t.c[b] = e.fold_c[c]; t.b8[b] = e.fold_b[c];
        t.b6[b] = wsum ? (int)((uint32_t)t.b8[b] - 2048u * (uint32_t)wsum[c] - ((uint32_t)kFoldMagicBits << 8)) : 0;
        if (e.bn_inv && e.bn_inv[c] < 0.0f) t.neg |= 1u << b;
    }
    return t;
}
// The table in device memory, in uint4 units: [slice][3][64 lanes] = {a0, a1, c0, c1}, {b8 of b = 0, 1, neg, 0},
// {b6 of b = 0, 1, neg, 0}: a form loads the first and the one of its matrix pipe, two coalesced 16-byte loads per lane.
constexpr int kHaloTabVec = 3 * 64;
__device__ __forceinline__ void qnn_halo_epi_tab_store(uint4* __restrict__ tab, int slice, int lane, const HaloEpiEntry& t) {
    uint4* o = tab + slice * kHaloTabVec + lane;
    o[0] = make_uint4(__float_as_uint(t.a[0]), __float_as_uint(t.a[1]), __float_as_uint(t.c[0]), __float_as_uint(t.c[1]));
    o[64] = make_uint4((uint32_t)t.b8[0], (uint32_t)t.b8[1], t.neg, 0u);
    o[128] = make_uint4((uint32_t)t.b6[0], (uint32_t)t.b6[1], t.neg, 0u);
}
template <bool FP6>
__device__ __forceinline__ HaloEpiEntry qnn_halo_epi_tab_load(const uint4* __restrict__ tab, int slice, int lane) {
    const uint4* o = tab + slice * kHaloTabVec + lane;
    const uint4 v0 = o[0], v1 = o[FP6 ? 128 : 64];
    HaloEpiEntry t;
    t.a[0] = __uint_as_float(v0.x); t.a[1] = __uint_as_float(v0.y);
    t.c[0] = __uint_as_float(v0.z); t.c[1] = __uint_as_float(v0.w);
    t.b8[0] = t.b6[0] = (int)v1.x; t.b8[1] = t.b6[1] = (int)v1.y;     // (the form reads only its own)
    t.neg = v1.z;
    return t;
}
#endif

// host side of the handle
struct qnn_fold {
    const qnn_weights* w;          // the layer it was built for
    int x_store, x_bits;
    const float* bn_inv;           // the epilogue it was built for (pointer identity is checked at launch)
    const float* bn_shift;
    int fn, act_bits, out_store;
    int has_res, res_store, res_bits;
    float post_scale;
    int cout;
    int mode;                      // 1: u = float(accw + beta) * A;  2 ("bits"): u = fma(as_float(accw + beta'), A, C);
                                   // 3 (image entry, x_store = QNN_STORE_U8): u = fma(float(S), A, C), no offset
    float* d_a;                    // [cout] slope
    int32_t* d_b;                  // [cout] offset, units of acc / 256 (mode 2: + 0x4B400000); mode 3: what the bits search
                                   // found for the table below (beta + 0x4B400000, or 0), reported only
    float* d_c;                    // [cout] mode 2: C = float(-12582912 * A); mode 1: zeros
    void* d_tab;                   // mode 3, usable, 64 filters: the first layer's operand table (kFirstTabVec uint4), or NULL
    void* d_halo_tab;              // mode 2, usable, 3x3 on 64 input channels, cout % 64 == 0 (the layers k_conv_mfma_halo takes): its
                                   // per-lane epilogue table (cout / 64 x kHaloTabVec uint4), or NULL
    int tab_bits;                  // the table carries the bits form (A', C', beta in the offset block) -- every channel passed
    int folded;                    // channels whose fold reproduced the chain on the whole domain
    long long points;
    int acc_lo, acc_hi;
};
