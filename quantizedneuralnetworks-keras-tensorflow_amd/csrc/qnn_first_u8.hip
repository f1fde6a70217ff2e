// First layer on the dataset's own bytes: x_store = QNN_STORE_U8, value = code / 255 (utils/load_data.py:40 forms the
// reference's float32 images exactly so).  Dispatch: route_first_u8 (qnn_conv.hip); any other shape with U8 input takes
// k_conv_generic, which implements the same arithmetic.
//
// With the integer weight codes k = w * 2^wshift the layer is an INTEGER problem with one offset:
//     s = code - 128  (one XOR with 0x80: a signed byte),     sum_k k s  +  128 sum_k k  =  sum_k k code  =  S
// -- ONE pass of v_mfma_i32_16x16x64_i8 per 16 positions x 16 filters.  A zero-padding tap is code 0, i.e. the byte
// -128, so the halo converts like any other pixel and sum_k k runs over all 27 taps regardless of the border: the
// constant 128 sum k is produced by the MFMA itself, in the K-block a 3x3x(3+1) window leaves empty (A bytes -128 from a
// constant LDS block, B bytes summing to -sum k).  The accumulator IS S.
// Everything the launch fuses behind the sum is one float32 FMA per value, t = fma(S, A[c], B[c]) (qnn_abi.h,
// qnn_conv2d_forward): the three digit passes, the 64 shift-adds and the four-rounding epilogue of the float-input
// fixed-point variant (qnn_first_fixed.hip) are gone, and the input is a quarter of the bytes.
//
// Layout (as qnn_first_fixed.hip): a wave walks a strip of 16 conv columns down the image two conv rows at a time.
// MFMA rows = 16 positions = 4 pool windows x (2 x 2), columns = 16 filters, K-block kq = tap row dy: 3 taps x
// (3 channels + 1 pad byte) + 4 bytes meeting zero weights; K-block 3 = the offset term.  Bytes are staged once
// (108 per step, two per lane) into a wave-private LDS ring of four input rows of 4-byte pixels.  In the C/D layout a
// lane holds the four positions of ONE window for one filter: pooling is an in-lane max on the integers (filters of
// channels with negative BN scale are negated, A[c] with them).
#include "qnn_mfma_common.h"
#include "qnn_fold.h"
#include "qnn_strip_plan.h"

namespace {

constexpr int kRowPitchU = 40;                 // words per LDS row (19 pixels touched; 40 == 8 mod 32)
constexpr int kRingU = 4 * kRowPitchU;         // ring of four input rows
constexpr int kConstU = kRingU;                // four words 0x80808080: the A operand of K-block 3
constexpr int kWaveLdsU = kRingU + 4;          // words per wave (a multiple of four: 16-byte aligned)

// F32IN (opt-in, input declared QNN_STORE_F32_IMAGE; route_first_img255): the same kernel for float32 inputs that ARE image bytes / 255
// (utils/load_data.py:40).  A staged value x is read as the byte k = rint(255 x) when |255 x - k| <= 2^-15 and
// 0 <= k <= 255 -- true for every float32 quotient k/255 (the product is off by < 2^-16) -- and raises the layer's
// domain flag otherwise (qnn_weights_check), exactly like the fixed-point variant.  An accepted x is within 1.5e-7 of
// k/255, so the result is within 27 * 1.5e-7 + one rounding of the real convolution of the floats: inside the 1e-5
// contract for anything the check lets through, and the typed entry's exact result for real images.
// Per element: t = 255 x (v_mul_f32, kept out of the packed-float form: v_pk_mul_f32 costs more than two plain
// multiplies beside MFMAs), u = t + 2^23 (rounds t to an integer k, ties to even as rint, and leaves k in the low bits of
// the sum), r0 = u - 2^23, z = bits(u) ^ 0x4B000080, d = t - r0.  The low byte of z is the signed byte the LDS takes
// (k ^ 0x80).  Nothing is decided per element: the lane keeps two running accumulators, orbits |= z and
// err = max(err, |d|), and the kernel tests them once at its end,  bad = (orbits & ~0xFF) != 0 || !(err <= 2^-15).
// That accepts and rejects exactly what the test against k clamped to [0, 255] did (|t - med3(r0, 0, 255)| <= 2^-15):
//   * bits 8..31 of z are zero exactly when u is one of the floats 2^23 + k, k = 0..255.  Then r0 = k, the clamp was
//     the identity, and both tests compare the same |t - k| with 2^-15 (a maximum over elements exceeds the bound
//     exactly when one element does; d is never NaN here).
//   * otherwise the bit test rejects, and so did the old test: u = NaN or +-inf has t = NaN or +-inf, whose distance
//     to any clamped value is NaN or inf; a finite u >= 2^23 + 256 needs t >= 255.5, at least 0.5 from the clamp's
//     255; a finite u < 2^23 needs t < -0.25 (2^23 - 0.25 is the tie, and it rounds to the even 2^23), more than 0.25
//     from the clamp's 0.  What v_max_f32 does with a NaN d is therefore irrelevant: its element already failed the
//     bit test.
struct ImageDomain {
    uint32_t orbits = 0u;
    float err = 0.0f;
    __device__ __forceinline__ bool bad() const { return (orbits & ~0xFFu) != 0u || !(err <= 0x1p-15f); }
};
// two staged elements at once: one v_or3_b32 and one v_max3_f32 serve both
__device__ __forceinline__ void image_bytes2(uint32_t& b0, uint32_t& b1, ImageDomain& dom) {
    float t0, t1, u0, u1;                        // (asm: the compiler pairs these into v_pk_mul_f32 / v_pk_add_f32)
    asm("v_mul_f32 %0, 0x437f0000, %1" : "=v"(t0) : "v"(__uint_as_float(b0)));
    asm("v_mul_f32 %0, 0x437f0000, %1" : "=v"(t1) : "v"(__uint_as_float(b1)));
    asm("v_add_f32 %0, 0x4b000000, %1" : "=v"(u0) : "v"(t0));
    asm("v_add_f32 %0, 0x4b000000, %1" : "=v"(u1) : "v"(t1));
    const float d0 = __fsub_rn(t0, __fsub_rn(u0, 8388608.0f)), d1 = __fsub_rn(t1, __fsub_rn(u1, 8388608.0f));
    b0 = __float_as_uint(u0) ^ 0x4B000080u;
    b1 = __float_as_uint(u1) ^ 0x4B000080u;
    dom.orbits |= b0 | b1;
    dom.err = fmaxf(fmaxf(dom.err, fabsf(d0)), fabsf(d1));
}

// three staged elements (the image-wide strip): the per-element arithmetic of image_bytes2, the two merges regrouped
__device__ __forceinline__ void image_bytes3(uint32_t& b0, uint32_t& b1, uint32_t& b2, ImageDomain& dom) {
    float t0, t1, t2, u0, u1, u2;
    asm("v_mul_f32 %0, 0x437f0000, %1" : "=v"(t0) : "v"(__uint_as_float(b0)));
    asm("v_mul_f32 %0, 0x437f0000, %1" : "=v"(t1) : "v"(__uint_as_float(b1)));
    asm("v_mul_f32 %0, 0x437f0000, %1" : "=v"(t2) : "v"(__uint_as_float(b2)));
    asm("v_add_f32 %0, 0x4b000000, %1" : "=v"(u0) : "v"(t0));
    asm("v_add_f32 %0, 0x4b000000, %1" : "=v"(u1) : "v"(t1));
    asm("v_add_f32 %0, 0x4b000000, %1" : "=v"(u2) : "v"(t2));
    const float d0 = __fsub_rn(t0, __fsub_rn(u0, 8388608.0f)), d1 = __fsub_rn(t1, __fsub_rn(u1, 8388608.0f));
    const float d2 = __fsub_rn(t2, __fsub_rn(u2, 8388608.0f));
    b0 = __float_as_uint(u0) ^ 0x4B000080u;
    b1 = __float_as_uint(u1) ^ 0x4B000080u;
    b2 = __float_as_uint(u2) ^ 0x4B000080u;
    dom.orbits = (dom.orbits | b0 | b1) | b2;
    dom.err = fmaxf(fmaxf(fmaxf(dom.err, fabsf(d0)), fabsf(d1)), fabsf(d2));
}

// (QNN_STORE_I4, 2, BIN): the fused pipeline, quantized_tanh / binary_tanh codes;  (QNN_STORE_F32, 1, false): the layer
// behind the float32 surface (any fn)
// FOLD (round 4): the epilogue of the pooled int4 form as qnn_fold.h's mode 3 -- u = fma(float(S), A2, C2), one
// v_cvt_pknorm_i16_f32 per pair, two v_perm_b32 + shift + v_bfi_b32 per eight values -- with A2 / C2 from a fold handle that
// qnn_fold_prepare accepted only after it reproduced  clip(rint(fma(float(S), A, B)))  on every S the filter can produce.
// TAB (with FOLD): 1 = the operands and constants come from the fold handle's table (qnn_fold.h, qnn_first_u8_entry: built once
// by qnn_fold_prepare with the function the preamble below calls) -- six 16-byte loads per lane, no LDS table, no workgroup
// barrier; 2 = that table carries the BITS form of the fold: the accumulator starts from a kept splat of 0x4B400000, the
// offset block's last A byte is +1 and meets beta[c], so the pooled maximum IS the bit pattern of the float
// 12582912 + S + beta (patterns of one binade order like the sums) and one FMA per value replaces conversion + FMA.
// 0 = the in-kernel preamble and the conversion (no handle, or QNN_EPI_NO_FIRST_TAB).
// SW: conv columns of a strip.  16 = the walk described above, any W % 16 == 0.  32 = the strip IS the row of a 32-pixel
// image (W == 32 only): two input rows are 192 values = three per lane with no dummy lane-slot, there is no column
// halo to load (ring pixels -1 and 32 keep the code-0 byte they are initialised with), no column test, one task per
// image and chunk, and a step is four tiles = 16 MFMAs whose epilogue runs per tile pair, (0, 1) then (2, 3).  The row
// pitch stays 40 words: the A reads touch pixels -1 .. 33 = 35 words, and 40 == 8 mod 32 keeps their banks.
template <int OUT, int POOL, bool BIN, bool F32IN, bool FOLD = false, int TAB = 0, int SW = 16>
__global__ __launch_bounds__(256, 4) void k_conv_first_u8(ConvGeom g, EpiArgs e, const void* __restrict__ x,
                                                           const float* __restrict__ wq, void* __restrict__ y,
                                                           int ntasks, int spr, FastDiv fd_spr, int nch, FastDiv fd_nch,
                                                           int rc, uint32_t img_x, float wscale, float D,
                                                           uint32_t* __restrict__ domain_flag) {
    extern __shared__ __attribute__((aligned(16))) char smem_u8[];
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wid = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
    uint32_t* lds = reinterpret_cast<uint32_t*>(smem_u8) + wave * kWaveLdsU;
    uint8_t* ldsb = reinterpret_cast<uint8_t*>(lds);
    static_assert(TAB == 0 || FOLD, "the operand table belongs to a fold handle");
    static_assert(SW == 16 || SW == 32, "a 16-column strip, or the whole row of a 32-pixel image");
    constexpr int NE = SW == 32 ? 3 : 2;                         // staged elements per lane and row pair
    constexpr int NT = SW / 8;                                   // tiles of 8 conv columns per step
    // code 0 everywhere; the constant block (bits form: its last byte is +1, the A byte that beta meets)
    for (int i = lane; i < kWaveLdsU; i += 64) lds[i] = (TAB == 2 && i == kConstU + 3) ? 0x01808080u : 0x80808080u;

    // ---- filters: B operand of block nt, column r, K-block kq.  Wave nt prepares block nt for the workgroup.
    // The pooled int4 forms DEAL the filters: column r of block nt is channel 4 r + nt, so the four blocks of a lane are
    // four consecutive channels of one pooled pixel = one 16-bit half of an output word, already in the order the
    // packing leaves them -- no transpose across lanes (the strip kernels' deal, qnn_mfma_strip.hip).  Everything
    // per-channel below (codes, the negation, A / B, the fold's A2 / C2) follows c. ----
    v4i bw[4];
    float fa[4], fb[4];
    if constexpr (TAB != 0) {
        const uint4* __restrict__ tb = reinterpret_cast<const uint4*>(e.first_tab);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) bw[nt] = __builtin_bit_cast(v4i, tb[nt * 64 + lane]);
        const uint4 ta = tb[4 * 64 + lane], tc = tb[5 * 64 + lane];
        fa[0] = __uint_as_float(ta.x); fa[1] = __uint_as_float(ta.y); fa[2] = __uint_as_float(ta.z); fa[3] = __uint_as_float(ta.w);
        fb[0] = __uint_as_float(tc.x); fb[1] = __uint_as_float(tc.y); fb[2] = __uint_as_float(tc.z); fb[3] = __uint_as_float(tc.w);
    } else {
        uint4* tab = reinterpret_cast<uint4*>(smem_u8 + 4 * kWaveLdsU * 4);  // [filter block][lane][2]
        const FirstU8Entry t = qnn_first_u8_entry<POOL == 2>(e, wq, wscale, D, wave, lane, FOLD ? e.fold_a : nullptr,
                                                             FOLD ? e.fold_c : nullptr, nullptr);
        tab[(wave * 64 + lane) * 2] = make_uint4(t.wd[0], t.wd[1], t.wd[2], t.wd[3]);
        tab[(wave * 64 + lane) * 2 + 1] = make_uint4(__float_as_uint(t.A), __float_as_uint(t.B), 0u, 0u);
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const uint4 t0 = tab[(nt * 64 + lane) * 2], t1 = tab[(nt * 64 + lane) * 2 + 1];
            bw[nt] = __builtin_bit_cast(v4i, t0);
            fa[nt] = __uint_as_float(t1.x); fb[nt] = __uint_as_float(t1.y);
        }
    }
    // the accumulators' initial value: zero, or (bits form) four registers kept for the whole kernel
    v4i z = {0, 0, 0, 0};
    if constexpr (TAB == 2) {
        z = v4i{kFoldMagicBits, kFoldMagicBits, kFoldMagicBits, kFoldMagicBits};
        asm volatile("" : "+v"(z));
    }
    constexpr int kMagicBits = 0x4B400008;                       // 1.5 * 2^23 + 8: see qnn_mfma_strip.hip
    const float magic = __int_as_float(kMagicBits);
    const int code_lo = kMagicBits - (int)e.act_m, code_hi = kMagicBits + (int)e.act_m - 1;
    // A lane's packed word P holds its four channels of tile 0 in the low half and of tile 1 in the high half.  Lanes r
    // and r ^ 1 hold the two halves of the same output words: one DPP exchange and one v_perm_b32 leave the even lane
    // with the whole word of tile 0 and the odd lane with that of tile 1.
    const uint32_t sel_join = (r & 1) ? 0x03020706u : 0x05040100u;
    auto join_tiles = [&](uint32_t P) { return __builtin_amdgcn_perm(dpp_xor1(P), P, sel_join); };
    // ---- operand addresses (dword index): position m = r: window w = r >> 2, (py, px) = bits of r.  A step works on
    // conv rows yy0 = 2*rp and yy0 + 1; with rp0 even the ring slot of input row yy0 + py + dy - 1 is
    // (2*(rp & 1) + py + kq) & 3.  K-block 3 reads the constant block for every tile ----
    const int py = (r >> 1) & 1, px = r & 1, w = r >> 2;
    const bool kconst = kq == 3;
    const int ab0 = kconst ? kConstU : ((py + kq) & 3) * kRowPitchU + 2 * w + px;            // + 8*t, + dx by the 4-dword read
    const int ab1 = kconst ? kConstU : ((2 + py + kq) & 3) * kRowPitchU + 2 * w + px;
    const int tstep = kconst ? 0 : 8;
    // ---- staging: two input rows = 108 bytes per step, elements lane and lane + 64 (lanes >= 44: a dummy pixel) ----
    const int e0row = lane >= 54 ? 1 : 0, e0rem = lane - 54 * e0row;
    const int e0px = e0rem / 3, e0ch = e0rem - 3 * e0px;
    const bool e1ok = lane < 44;
    const int e1rem = e1ok ? lane + 10 : 0;
    const int e1px = e1rem / 3, e1ch = e1rem - 3 * e1px;
    const int st0 = e0row * (kRowPitchU * 4) + e0px * 4 + e0ch;           // + slot * 160
    const int st1 = e1ok ? kRowPitchU * 4 + e1px * 4 + e1ch : kRowPitchU * 4 + 30 * 4;     // pixel 30 of a row is never read
    constexpr int EB = F32IN ? 4 : 1;                            // bytes per input element
    const int rowb = g.W * 3 * EB;                               // bytes per input row
    ImageDomain dom;                                             // F32IN: what this lane staged, tested once at the end
    // the wide strip: elements lane, lane + 64, lane + 128 of the 192 values of two whole rows, which are contiguous in
    // the image; ring pixel = column + 1.  Per-lane constants of the kernel, not of a task.
    int st[NE];
    const int vw = lane * EB;                                    // byte offset of element `lane` in a row pair
    if constexpr (SW == 32) {
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            const int idx = lane + 64 * j;
            const int erow = idx >= 96 ? 1 : 0, erem = idx - 96 * erow;
            const int epx = erem / 3, ech = erem - 3 * epx;
            st[j] = erow * (kRowPitchU * 4) + (epx + 1) * 4 + ech;
        }
    } else {
        st[0] = st0; st[1] = st1;
    }

    for (int task = wid; task < ntasks; task += nw) {
        const uint32_t rest = qnn_div((uint32_t)task, fd_nch);
        const int chunk = task - (int)rest * nch;
        const int n = SW == 32 ? (int)rest : (int)qnn_div(rest, fd_spr);
        const int xs = SW == 32 ? 0 : ((int)rest - n * spr) * 16;
        const int rp0 = chunk * rc, rp1 = min(rp0 + rc, g.H / 2);        // rc is even or nch == 1: rp0 is even
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
            (uint8_t*)const_cast<void*>(x) + (size_t)n * img_x, 0, (int)img_x, 0x00020000);
        // byte offsets of the two staged elements in input row 0 (the row offset is added below); columns outside the
        // image and, through the per-image descriptor, rows outside it read 0 = code 0
        // this lane's packed output word of a step (fused form): byte offset inside the image's output, the step's row
        // goes into the scalar offset of the store -- no per-step address arithmetic on the vector unit
        const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<uint32_t*>(y) + (size_t)n * g.Hp * g.Wp * e.ocw, 0, g.Hp * g.Wp * e.ocw * 4, 0x00020000);
        // (after join_tiles lane r holds word r >> 1 = channels 8 (r >> 1) .. + 7 of window kq in tile r & 1)
        const int ylane = (((xs >> 1) + kq + 4 * (r & 1)) * e.ocw + (r >> 1)) * 4;
        const int yrow = g.Wp * e.ocw * 4;
        const int c0col = xs - 1 + e0px, c1col = xs - 1 + e1px;
        const int v0 = (c0col >= 0 && c0col < g.W) ? (c0col * 3 + e0ch) * EB + e0row * rowb : (int)0x80000000;
        const int v1 = (e1ok && c1col >= 0 && c1col < g.W) ? (c1col * 3 + e1ch) * EB + rowb : (int)0x80000000;
        struct Staged { uint32_t b[NE]; };
        // wide strip: rows >= 0 need one sum per lane, elements 1 and 2 ride on the instruction's offset field; the
        // task's first load may start at row -1, and there each element's whole sum is formed so that it wraps as one
        auto stage_load = [&](int row, Staged& f, bool first = false) {      // rows `row`, `row + 1`
            const int so = row * rowb;                           // may be negative: the sum wraps out of range
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                int vo = (SW == 32 ? vw + 64 * j * EB : j == 0 ? v0 : v1) + so;
                if (SW == 32 && first) asm volatile("" : "+v"(vo));
                if constexpr (F32IN) f.b[j] = __builtin_amdgcn_raw_buffer_load_b32(xr, vo, 0, 0);   // float bits; converted at the write
                else f.b[j] = __builtin_amdgcn_raw_buffer_load_b8(xr, vo, 0, 0);
            }
        };
        auto stage_write = [&](auto slotc, Staged f) {           // into the ring slots SLOT, SLOT + 1
            constexpr int SB = decltype(slotc)::value * (kRowPitchU * 4);
            if constexpr (F32IN) {                               // the low bytes come back as signed bytes
                if constexpr (SW == 32) image_bytes3(f.b[0], f.b[1], f.b[2], dom);
                else image_bytes2(f.b[0], f.b[1], dom);
            } else {
#pragma unroll
                for (int j = 0; j < NE; ++j) f.b[j] ^= 0x80u;
            }
#pragma unroll
            for (int j = 0; j < NE; ++j) ldsb[st[j] + SB] = (uint8_t)f.b[j];
        };
        const int yy_first = 2 * rp0;
        Staged fsa, fsb, fsc;
        stage_load(yy_first - 1, fsa, true);
        stage_load(yy_first + 1, fsb);
        stage_load(yy_first + 3, fsc);
        stage_write(std::integral_constant<int, 0>{}, fsa);              // rows yy_first - 1, yy_first: slots 0, 1

        auto step = [&](auto parc, int rp) {
            constexpr int PAR = decltype(parc)::value;           // rp & 1
            const int yy0 = 2 * rp;
            // rows yy0+1, yy0+2 complete the four rows of this step: slots (yy0 + 2) & 3 and the next
            stage_write(std::integral_constant<int, PAR ? 0 : 2>{}, fsb);
            fsb = fsc;
            stage_load(yy0 + 5, fsc);                            // two steps ahead
            const uint32_t* abase = lds + (PAR ? ab1 : ab0);
            v4i A[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const uint32_t* p = abase + tstep * t;
                // the 4th dword (the pixel after the three taps) meets zero filter bytes
                A[t] = __builtin_bit_cast(v4i, make_uint4(p[0], p[1], p[2], p[3]));
            }
            // 4 NT groups (tile t = gq >> 2, filter block nt = gq & 3): the MFMA of group gq + 1 is issued before group gq
            // is consumed; the packing epilogue runs behind every eighth group, on tiles (0, 1) and (wide strip) (2, 3)
            constexpr int NG = 4 * NT;
            v4i acc[2];
            int T[8];
            auto consume = [&](int gq, const v4i& a) {
                const int t = gq >> 2, nt = gq & 3;
                if constexpr (POOL == 2) {
                    T[gq & 7] = max(max(a[0], a[1]), max(a[2], a[3]));
                } else {
                    // position i of window kq -> conv pixel (yy0 + (i >> 1), xs + 8t + 2kq + (i & 1))
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = nt * 16 + r;
                        float v = __fmaf_rn((float)a[i], fa[nt], fb[nt]);
                        if (e.fn == QNN_FN_BINARY_TANH) v = v > 0x1p-24f ? 1.0f : -1.0f;
                        else if (e.fn == QNN_FN_QUANTIZED_TANH)
                            v = __fmul_rn(fminf(fmaxf(rintf(v), -e.act_m), e.act_m - 1.0f),
                                          __uint_as_float(0x7F000000u - __float_as_uint(e.act_m)));
                        const long q = ((long)n * g.H + yy0 + (i >> 1)) * g.W + xs + 8 * t + 2 * kq + (i & 1);
                        reinterpret_cast<float*>(y)[q * g.cout + c] = v;
                    }
                }
            };
            acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[0], bw[0], z, 0, 0, 0);
#pragma unroll
            for (int h = 0; h < NT / 2; ++h) {
#pragma unroll
                for (int gq = 8 * h; gq < 8 * h + 8; ++gq) {
                    if (gq + 1 < NG)
                        acc[(gq + 1) & 1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[(gq + 1) >> 2], bw[(gq + 1) & 3], z, 0, 0, 0);
                    consume(gq, acc[gq & 1]);
                }
                // tile pair h: pooled pixels kq + 4 * tile start 8 further per pair = 8 * ocw words, on the store's scalar offset
                const int ys = rp * yrow + h * (32 * e.ocw);
                if constexpr (OUT == QNN_STORE_I4 && FOLD) {
                    static_assert(!FOLD || (!BIN && POOL == 2), "the fold covers the pooled quantized_tanh form");
                    uint32_t tp[4];
    #pragma unroll
                    for (int j = 0; j < 4; ++j)             // pairs (value j, value j + 4): same filter block, tiles 0 and 1
                        tp[j] = TAB == 2 ? qnn_fold_pair_bits(T[j], T[j + 4], fa[j], fa[j], fb[j], fb[j])
                                         : qnn_fold_pair_fma(T[j], T[j + 4], fa[j], fa[j], fb[j], fb[j]);
                    const uint32_t uo = __builtin_amdgcn_perm(tp[3], tp[1], 0x07030501u);
                    const uint32_t ue = __builtin_amdgcn_perm(tp[2], tp[0], 0x07030501u);
                    const uint32_t P = (uo & 0xF0F0F0F0u) | ((ue >> 4) & 0x0F0F0F0Fu);      // nibble j = code of value j
                    __builtin_amdgcn_raw_buffer_store_b32(join_tiles(P), yr, ylane, ys, 0);
                } else if constexpr (OUT == QNN_STORE_I4) {
                    // lane (column r, window kq): value j = 4*t + nt = channel 4 r + nt of pooled pixel xs/2 + kq + 4 t
                    int cb[8];
    #pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float u = __fmaf_rn((float)T[j], fa[j & 3], fb[j & 3]);
                        if constexpr (BIN) {
                            cb[j] = u > 0x1p-24f ? kMagicBits + 1 : kMagicBits - 1;
                        } else {
                            // rint + clamp in one add and one integer median (the low bits of u + magic are rint(u) + 8)
                            const int bits = __float_as_int(__fadd_rn(u, magic));
                            asm("v_med3_i32 %0, %1, %2, %3" : "=v"(cb[j]) : "v"(bits), "v"(code_lo), "v"(code_hi));
                        }
                    }
                    // sum_j cb[j] << 4j by Horner: seven v_lshl_add_u32 (the compiler's form was 7 shifts + 5 three-way adds)
                    uint32_t P = (uint32_t)cb[7];
    #pragma unroll
                    for (int j = 6; j >= 0; --j) asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(P) : "v"(P), "v"(cb[j]));
                    P -= (uint32_t)(kMagicBits - 8) * 0x11111111u;
                    const uint32_t Wd = join_tiles(P) ^ 0x88888888u;
                    __builtin_amdgcn_raw_buffer_store_b32(Wd, yr, ylane, ys, 0);
                }
            }
        };
        int rp = rp0;
        for (; rp + 2 <= rp1; rp += 2) {
            step(std::integral_constant<int, 0>{}, rp);
            step(std::integral_constant<int, 1>{}, rp + 1);
        }
        if (rp < rp1) step(std::integral_constant<int, 0>{}, rp);
    }
    if constexpr (F32IN) {
        if (dom.bad()) *domain_flag = 1u;    // reported by qnn_weights_check / the next qnn_conv2d_forward, never silent
    }
}


// ---------------------------------------------------------------------------------------------------------------
// The same layer WITHOUT pooling and with packed output: the first conv of a deeper stage (VGG with nla > 1: 3 -> 64 ...
// 256 filters, int4 or int8 codes) and the ResNet stem (3 -> 16, models/resnet.py:96-99).  Same strip walk, staging and
// MFMA; every conv position is stored, so the epilogue runs on all 2048 results of a step (not on 512 pooled ones) and
// the offset term 128 * sum k is added as an integer (an 8-bit filter's sum does not fit the sixteen spare bytes).
// A wave computes NBLK blocks of 16 filters (blockIdx.y selects the slice of 16 * NBLK).  Packing: int8 -- a 4 x 4 byte
// transpose over a lane quad leaves lane (r & 3) = position with four consecutive filters; int4 -- an 8 x 8 nibble
// transpose over a lane octet pairs two filter blocks (NBLK = 4) or the step's two tiles (NBLK = 1) so that every lane
// ends with one pixel's eight consecutive channels.  One dword store per lane and group.
// (16 filters per wave = two MFMAs per step: little to overlap inside a wave, so that form runs six workgroups per CU)
template <int OUT, int NBLK, bool BIN, bool F32IN>
__global__ __launch_bounds__(256, (NBLK == 1 ? 6 : 3)) void k_conv_first_u8_full(ConvGeom g, EpiArgs e, const void* __restrict__ x,
                                                                const float* __restrict__ wq, void* __restrict__ y,
                                                                int ntasks, int spr, FastDiv fd_spr, int nch, FastDiv fd_nch,
                                                                int rc, uint32_t img_x, float wscale, float D,
                                                                uint32_t* __restrict__ domain_flag) {
    static_assert(OUT == QNN_STORE_I4 || OUT == QNN_STORE_I8, "packed outputs");
    static_assert(NBLK == 1 || NBLK == 4, "16 or 64 filters per wave");
    extern __shared__ __attribute__((aligned(16))) char smem_u8[];
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // Workgroup -> (task stream xw, filter slice): the slices of one task stream sit on ONE XCD (workgroups are dealt to
    // the eight XCDs round robin) and start together, so the 64-byte pieces of a stored pixel that different slices write
    // meet in the same L2 instead of leaving four partial lines in four of them.  gridDim.y = slices, gridDim.x % 8 == 0
    // (otherwise the plain mapping).
    const int nsl = gridDim.y, bxw = gridDim.x;
    const int bid = blockIdx.y * bxw + blockIdx.x;
    int xw = blockIdx.x, slice = blockIdx.y;
    if ((bxw & 7) == 0 && nsl > 1) {
        const int xcd = bid & 7, j = bid >> 3;
        slice = j % nsl;
        xw = (j / nsl) * 8 + xcd;
    }
    const int wid = xw * 4 + wave, nw = bxw * 4;
    const int cbase = slice * (16 * NBLK);
    uint32_t* lds = reinterpret_cast<uint32_t*>(smem_u8) + wave * kWaveLdsU;
    uint8_t* ldsb = reinterpret_cast<uint8_t*>(lds);
    uint4* tab = reinterpret_cast<uint4*>(smem_u8 + 4 * kWaveLdsU * 4);      // [filter block][lane][2]
    for (int i = lane; i < kWaveLdsU; i += 64) lds[i] = 0x80808080u;

    // int8 output of 64 filters per workgroup: the MFMA operands swap roles (rows = filters, columns = positions), and the
    // rows of filter block nt are the filters 16 * (row >> 2) + 4 * nt + (row & 3): a lane then ends with the SIXTEEN
    // CONSECUTIVE filters cbase + 16 kq .. + 15 of one position = one 16-byte store, no lane transposes.  (The 4-byte
    // stores of the other form, 16-byte runs 256 bytes apart, kept this layer at 0.68 ms for 1.07 GB on VGG-large.)
    constexpr bool SWAP = OUT == QNN_STORE_I8 && NBLK == 4;
    if (wave < NBLK) {
        const int c = SWAP ? cbase + 16 * (r >> 2) + 4 * wave + (r & 3) : cbase + wave * 16 + r;
        const float bias = e.bias ? e.bias[c] : 0.0f;
        const float inv = e.bn_inv ? e.bn_inv[c] : 1.0f;
        const float shift = e.bn_inv ? e.bn_shift[c] : 0.0f;
        const float* wrow = wq + (size_t)c * 27 + (kq < 3 ? kq : 2) * 9;
        int part = 0;
        uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            int code = (int)rintf(__fmul_rn(wrow[i], wscale));
            if (kq == 3) code = 0;
            part += code;
            wd[i / 3] |= (uint32_t)(code & 0xFF) << (8 * (i % 3));
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        const double m = e.fn == QNN_FN_QUANTIZED_TANH ? (double)e.act_m : 1.0;
        const float A = (float)((double)inv * m / (double)D);
        const float B = (float)(((double)bias * (double)inv + (double)shift) * m);
        tab[(wave * 64 + lane) * 2] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        tab[(wave * 64 + lane) * 2 + 1] = make_uint4(__float_as_uint(A), __float_as_uint(B), (uint32_t)(128 * part), 0u);
    }
    __syncthreads();
    v4i bw[NBLK];
    float fa[NBLK], fb[NBLK];
    int c0[NBLK];
#pragma unroll
    for (int nt = 0; nt < NBLK; ++nt) {
        const uint4 t0 = tab[(nt * 64 + lane) * 2], t1 = tab[(nt * 64 + lane) * 2 + 1];
        bw[nt] = __builtin_bit_cast(v4i, t0);
        fa[nt] = __uint_as_float(t1.x); fb[nt] = __uint_as_float(t1.y); c0[nt] = (int)t1.z;
    }
    float fa16[SWAP ? 16 : 1], fb16[SWAP ? 16 : 1];
    int c16[SWAP ? 16 : 1];
    if constexpr (SWAP) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {                 // filter cbase + 16 kq + j = row 4 kq + (j & 3) of block j >> 2
            const uint4 t1 = tab[((j >> 2) * 64 + 4 * kq + (j & 3)) * 2 + 1];
            fa16[j] = __uint_as_float(t1.x); fb16[j] = __uint_as_float(t1.y); c16[j] = (int)t1.z;
        }
    }
    LaneEpi ke;
    lane_epi_init<OUT>(ke, e, r, r);
    const int py = (r >> 1) & 1, px = r & 1, w = r >> 2;
    const bool kconst = kq == 3;
    const int ab0 = kconst ? kConstU : ((py + kq) & 3) * kRowPitchU + 2 * w + px;
    const int ab1 = kconst ? kConstU : ((2 + py + kq) & 3) * kRowPitchU + 2 * w + px;
    const int tstep = kconst ? 0 : 8;
    const int e0row = lane >= 54 ? 1 : 0, e0rem = lane - 54 * e0row;
    const int e0px = e0rem / 3, e0ch = e0rem - 3 * e0px;
    const bool e1ok = lane < 44;
    const int e1rem = e1ok ? lane + 10 : 0;
    const int e1px = e1rem / 3, e1ch = e1rem - 3 * e1px;
    const int st0 = e0row * (kRowPitchU * 4) + e0px * 4 + e0ch;
    const int st1 = e1ok ? kRowPitchU * 4 + e1px * 4 + e1ch : kRowPitchU * 4 + 30 * 4;
    constexpr int EB = F32IN ? 4 : 1;
    const int rowb = g.W * 3 * EB;
    ImageDomain dom;
    // ---- where this lane's packed word of a group goes: position jj of window kq (tile t: + 8 columns) ----
    const int jj = (OUT == QNN_STORE_I8) ? (r & 3) : (r & 3);          // after the transposes a lane holds position r & 3
    const int pixb = e.ocw * 4;                                        // bytes per stored pixel
    // int8: four consecutive filters from r & ~3;  int4: eight from r & 8, block (or tile) selected by bit 2 of r
    const int chan_b = (OUT == QNN_STORE_I8) ? (r & ~3) : ((r & 8) >> 1);
    const int hi = (r >> 2) & 1;                                       // int4: second block / second tile of the pair

    for (int task = wid; task < ntasks; task += nw) {
        const uint32_t rest = qnn_div((uint32_t)task, fd_nch);
        const int chunk = task - (int)rest * nch;
        const int n = (int)qnn_div(rest, fd_spr);
        const int xs = ((int)rest - n * spr) * 16;
        const int rp0 = chunk * rc, rp1 = min(rp0 + rc, g.H / 2);
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
            (uint8_t*)const_cast<void*>(x) + (size_t)n * img_x, 0, (int)img_x, 0x00020000);
        const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<uint8_t*>(y) + (size_t)n * g.H * g.W * pixb, 0, g.H * g.W * pixb, 0x00020000);
        // byte offset of this lane's word for tile 0 of conv row pair 0 (NBLK = 1, int4: the lane's tile is `hi`)
        const int ycol = xs + 2 * kq + (jj & 1) + ((OUT == QNN_STORE_I4 && NBLK == 1) ? 8 * hi : 0);
        const int ylane = ((jj >> 1) * g.W + ycol) * pixb + cbase * (OUT == QNN_STORE_I8 ? 1 : 0) + (OUT == QNN_STORE_I4 ? cbase / 2 : 0) + chan_b;
        const int yrow2 = 2 * g.W * pixb;                               // two conv rows per step
        const int c0col = xs - 1 + e0px, c1col = xs - 1 + e1px;
        const int v0 = (c0col >= 0 && c0col < g.W) ? (c0col * 3 + e0ch) * EB + e0row * rowb : (int)0x80000000;
        const int v1 = (e1ok && c1col >= 0 && c1col < g.W) ? (c1col * 3 + e1ch) * EB + rowb : (int)0x80000000;
        auto stage_load = [&](int row, uint32_t& b0, uint32_t& b1) {
            const int so = row * rowb;
            if constexpr (F32IN) {
                b0 = __builtin_amdgcn_raw_buffer_load_b32(xr, v0 + so, 0, 0);
                b1 = __builtin_amdgcn_raw_buffer_load_b32(xr, v1 + so, 0, 0);
            } else {
                b0 = __builtin_amdgcn_raw_buffer_load_b8(xr, v0 + so, 0, 0);
                b1 = __builtin_amdgcn_raw_buffer_load_b8(xr, v1 + so, 0, 0);
            }
        };
        auto stage_write = [&](auto slotc, uint32_t b0, uint32_t b1) {
            constexpr int SB = decltype(slotc)::value * (kRowPitchU * 4);
            if constexpr (F32IN) image_bytes2(b0, b1, dom);      // the low bytes come back as signed bytes
            else { b0 ^= 0x80u; b1 ^= 0x80u; }
            ldsb[st0 + SB] = (uint8_t)b0;
            ldsb[st1 + SB] = (uint8_t)b1;
        };
        const int yy_first = 2 * rp0;
        uint32_t fa0, fa1, fb0, fb1, fc0, fc1;
        stage_load(yy_first - 1, fa0, fa1);
        stage_load(yy_first + 1, fb0, fb1);
        stage_load(yy_first + 3, fc0, fc1);
        stage_write(std::integral_constant<int, 0>{}, fa0, fa1);

        auto step = [&](auto parc, int rp) {
            constexpr int PAR = decltype(parc)::value;
            const int yy0 = 2 * rp;
            stage_write(std::integral_constant<int, PAR ? 0 : 2>{}, fb0, fb1);
            fb0 = fc0; fb1 = fc1;
            stage_load(yy0 + 5, fc0, fc1);
            const uint32_t* abase = lds + (PAR ? ab1 : ab0);
            v4i A[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const uint32_t* p = abase + tstep * t;
                A[t] = __builtin_bit_cast(v4i, make_uint4(p[0], p[1], p[2], p[3]));
            }
            const v4i z = {0, 0, 0, 0};
            const int srow = rp * yrow2;                            // scalar offset of the step's rows
            // t = fma(S, A, B) of the four positions of window kq for filter block nt (pre-scaled by the code scale)
            auto values = [&](const v4i& a, int nt, float* tv) {
#pragma unroll
                for (int i = 0; i < 4; ++i) tv[i] = __fmaf_rn((float)(a[i] + c0[nt]), fa[nt], fb[nt]);
            };
            if constexpr (SWAP) {
                // position r of tile t: conv row 2 rp + py, column xs + 8 t + 2 w + px
                const int ypos = (py * g.W + xs + 2 * w + px) * pixb + cbase + 16 * kq;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    uint32_t Pq[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        const v4i a = __builtin_amdgcn_mfma_i32_16x16x64_i8(bw[nt], A[t], z, 0, 0, 0);
                        float tv[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            tv[i] = __fmaf_rn((float)(a[i] + c16[4 * nt + i]), fa16[4 * nt + i], fb16[4 * nt + i]);
                        Pq[nt] = pack_scaled<8, 4>(tv, e.act_m, BIN) ^ 0x80808080u;
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, make_uint4(Pq[0], Pq[1], Pq[2], Pq[3])), yr,
                                                           ypos + (8 * t) * pixb, srow, 0);
                    // A 16-byte store reads its data VGPRs a state after issue, and hipcc inserts no wait state here:
                    // in the F32IN forms the very next instruction rewrote the first data register, and that dword of
                    // some stores came out wrong, nondeterministically.  The fences keep the nop right behind the store.
                    __builtin_amdgcn_sched_barrier(0);
                    asm volatile("s_nop 1");
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else if constexpr (OUT == QNN_STORE_I8) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int nt = 0; nt < NBLK; ++nt) {
                        const v4i a = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], bw[nt], z, 0, 0, 0);
                        float tv[4];
                        values(a, nt, tv);
                        const uint32_t P = pack_scaled<8, 4>(tv, e.act_m, BIN);
                        const uint32_t Wd = transpose_byte4(P, ke) ^ 0x80808080u;
                        __builtin_amdgcn_raw_buffer_store_b32(Wd, yr, ylane + (8 * t) * pixb + nt * 16, srow, 0);
                    }
            } else if constexpr (NBLK == 4) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int np = 0; np < 2; ++np) {                // filter blocks 2*np, 2*np + 1 share a word
                        const v4i a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], bw[2 * np], z, 0, 0, 0);
                        const v4i a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], bw[2 * np + 1], z, 0, 0, 0);
                        float tv[8];
                        values(a0, 2 * np, tv);
                        values(a1, 2 * np + 1, tv + 4);
                        const uint32_t P = pack_scaled<4, 8>(tv, e.act_m, BIN);
                        const uint32_t Wd = transpose_nib8(P, ke) ^ 0x88888888u;
                        __builtin_amdgcn_raw_buffer_store_b32(Wd, yr, ylane + (8 * t) * pixb + (2 * np + hi) * 8, srow, 0);
                    }
            } else {
                const v4i a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[0], bw[0], z, 0, 0, 0);      // tile 0, tile 1
                const v4i a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[1], bw[0], z, 0, 0, 0);
                float tv[8];
                values(a0, 0, tv);
                values(a1, 0, tv + 4);
                const uint32_t P = pack_scaled<4, 8>(tv, e.act_m, BIN);
                const uint32_t Wd = transpose_nib8(P, ke) ^ 0x88888888u;
                __builtin_amdgcn_raw_buffer_store_b32(Wd, yr, ylane, srow, 0);
            }
        };
        int rp = rp0;
        for (; rp + 2 <= rp1; rp += 2) {
            step(std::integral_constant<int, 0>{}, rp);
            step(std::integral_constant<int, 1>{}, rp + 1);
        }
        if (rp < rp1) step(std::integral_constant<int, 0>{}, rp);
    }
    if constexpr (F32IN) {
        if (dom.bad()) *domain_flag = 1u;
    }
}

}  // namespace

// 0 = launched.  3x3, stride 1, SAME, 3 input channels, 64 filters of <= 7 bits (or binary), W % 16 == 0, H even;
// fused pipeline form (pool 2, int4 codes out) or float32 output without pooling.
int qnn_try_launch_first_u8(const ConvGeom& g, const EpiArgs& e, const void* x, const qnn_weights* w, void* y,
                            hipStream_t s, bool f32in) {
    if (f32in && !(e.dom_flag ? e.dom_flag : w->d_flag)) return 1;                           // no flag word, no restricted-domain kernel
    if (g.kh != 3 || g.kw != 3 || g.stride != 1 || g.pt != 1 || g.pl != 1 || g.cin != 3 || e.res) return 1;
    if ((g.W % 16) != 0 || (g.H % 2) != 0 || !w->d_wq) return 1;
    // weight codes = value * 2^wshift: binary (+-1, H = 1) or quantized (pooled form: <= 7 bits, |code| <= 64 -- the negated
    // filter still fits a signed byte and sixteen bytes hold -sum k; un-pooled packed form: <= 8 bits)
    if (w->wkind == QNN_W_BINARY ? (w->H != 1.0f || w->wshift != 0)
                               : (w->wkind != QNN_W_QUANT || w->wshift < 1 || w->wshift > 7)) return 1;
    const bool small_codes = w->wshift <= 6;
    const bool ok_fused = g.cout == 64 && small_codes && g.pool == 2 && e.out_store == QNN_STORE_I4 &&
                          ((e.fn == QNN_FN_QUANTIZED_TANH && e.act_m <= 8.0f) || e.fn == QNN_FN_BINARY_TANH);
    const bool rawf = g.cout == 64 && small_codes && g.pool == 1 && e.out_store == QNN_STORE_F32 &&
                      (e.fn == QNN_FN_NONE || e.fn == QNN_FN_QUANTIZED_TANH || e.fn == QNN_FN_BINARY_TANH);
    // un-pooled packed output (k_conv_first_u8_full): 16 filters (ResNet stem) or a multiple of 64
    const bool ok_full = g.pool == 1 && (e.out_store == QNN_STORE_I4 || e.out_store == QNN_STORE_I8) &&
                         (g.cout == 16 || (g.cout % 64) == 0) &&
                         ((e.fn == QNN_FN_QUANTIZED_TANH && e.act_m <= (e.out_store == QNN_STORE_I4 ? 8.0f : 128.0f)) ||
                          e.fn == QNN_FN_BINARY_TANH);
    if (!ok_fused && !rawf && !ok_full) return 1;
    const float wscale = (float)(1 << w->wshift);
    const int spr = g.W / 16;
    const double img_x = (double)g.H * g.W * 3 * (f32in ? 4 : 1);
    const float D = 255.0f * wscale;                             // the divisor of the affine map (qnn_abi.h)
    if (img_x >= 1.0e9 || (double)g.N * g.Hp * g.Wp * 8.0 >= 2.0e9 * 4) return 1;
    const bool fused = g.cout == 64 && w->wshift <= 6 && g.pool == 2 && e.out_store == QNN_STORE_I4 &&
                       ((e.fn == QNN_FN_QUANTIZED_TANH && e.act_m <= 8.0f) || e.fn == QNN_FN_BINARY_TANH);
    const bool full = !fused && g.pool == 1 && e.out_store != QNN_STORE_F32;
    // persistent grid = what is resident: four workgroups per CU (three for the un-pooled packed form, launch bounds)
    const int blocks_cap = 256 * (full ? (g.cout == 16 ? 6 : 3) : 4);
    // the walk is over row pairs, an even number per task (every chunk starts on an even row pair); 1.5 pairs of fill
    StripPlan p;
    if (!qnn_strip_plan(&p, g.N, spr, g.H / 2, blocks_cap, 1.5, 2)) return 1;
    const dim3 grid(p.blocks), block(256);
    const size_t lds = (size_t)4 * kWaveLdsU * 4 + 4 * 64 * 2 * 16;
    if (full && !fused) {
        if ((double)g.H * g.W * e.ocw * 4.0 >= 2.0e9) return 1;
        const int nblk = g.cout == 16 ? 1 : 4;
        const int gy = g.cout / (16 * nblk);
        long bx = blocks_cap / gy > 0 ? blocks_cap / gy : 1;
        if (bx > (p.ntasks + 3L) / 4) bx = (p.ntasks + 3L) / 4;
        const dim3 fgrid((unsigned)bx, (unsigned)gy);
        const bool bin = e.fn == QNN_FN_BINARY_TANH;
#define U8_FULL(OUT_, NB_, BIN_, F32_)                                                                                      \
        hipLaunchKernelGGL((k_conv_first_u8_full<OUT_, NB_, BIN_, F32_>), fgrid, block, lds, s, g, e, x, w->d_wq, y,         \
                           QNN_STRIP_PLAN_ARGS(p), (uint32_t)img_x, wscale, D, (e.dom_flag ? e.dom_flag : w->d_flag))
#define U8_FULL_B(OUT_, NB_)                                                                                                \
        do {                                                                                                               \
            if (bin) { if (f32in) U8_FULL(OUT_, NB_, true, true); else U8_FULL(OUT_, NB_, true, false); }                   \
            else { if (f32in) U8_FULL(OUT_, NB_, false, true); else U8_FULL(OUT_, NB_, false, false); }                     \
        } while (0)
        if (e.out_store == QNN_STORE_I8) { if (nblk == 1) U8_FULL_B(QNN_STORE_I8, 1); else U8_FULL_B(QNN_STORE_I8, 4); }
        else { if (nblk == 1) U8_FULL_B(QNN_STORE_I4, 1); else U8_FULL_B(QNN_STORE_I4, 4); }
#undef U8_FULL_B
#undef U8_FULL
        return 0;
    }
    // W == 32: the strip is the whole row (SW = 32), one task per image and chunk -- same planner, same LDS, same name in
    // the kernel log.  QNN_EPI_NO_FIRST_WIDE keeps the two 16-column strips; every other width has only those.
    const bool wide = g.W == 32 && !(e.flags & QNN_EPI_NO_FIRST_WIDE);
    if (wide && !qnn_strip_plan(&p, g.N, 1, g.H / 2, blocks_cap, 1.5, 2)) return 1;
    const dim3 wgrid(p.blocks);
    const size_t lds_ring = (size_t)4 * kWaveLdsU * 4;           // the table forms keep no operand table in LDS
    uint32_t* const dflag = e.dom_flag ? e.dom_flag : w->d_flag;
#define U8_K(OUT_, POOL_, BIN_, F32_, FOLD_, TAB_, LDS_)                                                                    \
    do {                                                                                                                   \
        if (!wide)                                                                                                         \
            hipLaunchKernelGGL((k_conv_first_u8<OUT_, POOL_, BIN_, F32_, FOLD_, TAB_>), grid, block, LDS_, s, g, e, x,      \
                               w->d_wq, y, QNN_STRIP_PLAN_ARGS(p), (uint32_t)img_x, wscale, D, dflag);                     \
        else                                                                                                               \
            hipLaunchKernelGGL((k_conv_first_u8<OUT_, POOL_, BIN_, F32_, FOLD_, TAB_, 32>), wgrid, block, LDS_, s, g, e, x, \
                               w->d_wq, y, QNN_STRIP_PLAN_ARGS(p), (uint32_t)img_x, wscale, D, dflag);                     \
    } while (0)
#define U8_LAUNCH(OUT_, POOL_, BIN_, FOLD_, TAB_, LDS_)                                                                     \
    do {                                                                                                                   \
        if (f32in) U8_K(OUT_, POOL_, BIN_, true, FOLD_, TAB_, LDS_);                                                        \
        else U8_K(OUT_, POOL_, BIN_, false, FOLD_, TAB_, LDS_);                                                             \
    } while (0)
    if (!fused) U8_LAUNCH(QNN_STORE_F32, 1, false, false, 0, lds);
    else if (e.fn == QNN_FN_BINARY_TANH) U8_LAUNCH(QNN_STORE_I4, 2, true, false, 0, lds);
    else if (e.fold_a && e.fold_c && e.act_m == 8.0f && e.first_tab) {     // ... with the handle's operand table
        if (e.first_tab_bits) U8_LAUNCH(QNN_STORE_I4, 2, false, true, 2, lds_ring);
        else U8_LAUNCH(QNN_STORE_I4, 2, false, true, 1, lds_ring);
    }
    // folded epilogue (mode 3 handle of this layer, qnn_fold.h)
    else if (e.fold_a && e.fold_c && e.act_m == 8.0f) U8_LAUNCH(QNN_STORE_I4, 2, false, true, 0, lds);
    else U8_LAUNCH(QNN_STORE_I4, 2, false, false, 0, lds);
#undef U8_LAUNCH
#undef U8_K
    return 0;
}
