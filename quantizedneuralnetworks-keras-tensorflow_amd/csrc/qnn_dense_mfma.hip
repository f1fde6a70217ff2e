// Hidden dense layers on the int8 matrix pipe: a register-fed GEMM on v_mfma_i32_16x16x64_i8.
//
// Reference ops replaced: BinaryDense.call (layers/binary_layers.py:78-85) and QuantizedDense.call
// (layers/quantized_layers.py:79-88) where route_dense (qnn_conv.hip) declines them: a packed output, or more than 256
// units.  Before this file such a call ran on k_conv_ps up to 64 input features and on k_conv_generic beyond.
//
// Both operands are stored K-major (x: [N][kwords], d_packed: [units][kwords]), which is the per-lane operand layout of
// the instruction, so nothing is staged: in K-step s lane (r = lane & 15, h = lane >> 4) loads the quarter h of the 64
// features of row r straight into the operand registers,
//   I8   16 bytes, the operand as stored;
//   I4   8 bytes, widened to 16 bytes of 16 * code (strip_widen; both operands alike, x 256 goes into the output scale);
//   BIN  16 bits, spread to 16 bytes of +-1 (cin % 64 == 0: no pad bits).
// A = weights (rows = units), B = activations (columns = images): after the MFMA a lane owns four consecutive units of
// one image, i.e. one 2-byte store of int4 codes, one dword of int8 codes or one float4: no transpose, no cross-lane
// packing.  A wave's tile is 16 images x 16 * NT units; each tile of weights beyond the first re-uses the wave's
// activation registers.  Loads run two K-steps ahead of the MFMAs through a ring of three register sets.  Every wave
// reads its rows through buffer descriptors that end with its tile: rows past N or past `units` read as zero and are
// never stored.
//
// Split-K inside the workgroup: the four waves are ks x (4 / ks); ks waves share one output tile and walk contiguous
// shares of ceil(steps / ks) K-steps (the last share may be short or empty), the other factor spreads the waves over
// image tiles.  The partial accumulators meet in LDS (at most 3 waves x NT x 1 KiB = 12 KiB) and are added as integers,
// so every ks gives the same bits.  NT and ks come from the host plan (dense_plan, qnn_dense_plan.h); there is no
// run-time switch.
//
// Epilogue: the chain of k_conv_generic from the same device functions in the same order -- __fmul_rn((float)acc, scale),
// qnn_epi_value, then qnn_binary_tanh / qnn_qact (float32 output) or qnn_epi_code (packed) -- so the bits are the generic
// kernel's.  units % 16 == 0 fills every int4 half-word and int8 dword: no spare bits.
//
// Registers (hipcc -O3, gfx950), the same for every operand store and output within a VGPR or two: NT = 1: 40 VGPRs + 8
// AGPRs (8 waves per SIMD), NT = 2: 61 + 16 (6 waves), NT = 4: 84 + 32 (4 waves); no scratch in any instantiation.
// LDS 3 / 6 / 12 KiB.  Measured times: profiles/dense_mfma/README.md.
#include <stdio.h>

#include "qnn_dense_plan.h"
#include "qnn_strip_device.h"

namespace {

// bytes of one row in one K-step (64 features); a lane loads a quarter of them
template <int XS>
constexpr int kStepBytes = XS == QNN_STORE_I8 ? 64 : XS == QNN_STORE_I4 ? 32 : 8;

template <int XS>
__device__ __forceinline__ auto dense_load(__amdgpu_buffer_rsrc_t rsrc, int off) {
    if constexpr (XS == QNN_STORE_I8) return __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
    else if constexpr (XS == QNN_STORE_I4) return __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0);
    else return __builtin_amdgcn_raw_buffer_load_b16(rsrc, off, 0, 0);
}

// what a lane loaded -> its 16 int8 operand bytes
template <int XS, typename Raw>
__device__ __forceinline__ v4i dense_operand(Raw raw) {
    if constexpr (XS == QNN_STORE_I8) {
        return __builtin_bit_cast(v4i, raw);
    } else if constexpr (XS == QNN_STORE_I4) {
        return strip_widen(make_uint2(raw[0], raw[1]));
    } else {
        // four bits -> four bytes: the multiply puts bit j at bit 8 j, x 0xFE makes the bytes 0 / -2, the xor -1 / +1
        auto four = [](uint32_t n) { return ((((n & 15u) * 0x00204081u) & 0x01010101u) * 0xFEu) ^ 0xFFFFFFFFu; };
        const uint32_t b = raw;
        return __builtin_bit_cast(v4i, make_uint4(four(b), four(b >> 4), four(b >> 8), four(b >> 12)));
    }
}

// rows [row0, row0 + tile_rows) of a K-major matrix of `rows` rows, as a buffer that ends where they end
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dense_rows_rsrc(const uint8_t* base, long row0, int tile_rows, long rows,
                                                                  int row_bytes) {
    const long left = rows - row0;
    const int have = left < 0 ? 0 : left < tile_rows ? (int)left : tile_rows;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base) + (have ? (size_t)row0 * row_bytes : 0), 0,
                                             have * row_bytes, 0x00020000);
}

template <int XS, int OUT, int NT>
__global__ __launch_bounds__(256) void k_dense_mfma(const uint8_t* __restrict__ x, const uint8_t* __restrict__ wp, EpiArgs e,
                                                    void* __restrict__ y, int N, int units, int steps, int ks, int ublocks) {
    constexpr int SB = kStepBytes<XS>;
    __shared__ v4i meet[3 * NT * 64];
    const int lane = threadIdx.x & 63, r = lane & 15, h = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int per = 4 / ks;                                  // image tiles of this workgroup
    const int kp = wave % ks, it = wave / ks;
    const int ub = blockIdx.x % ublocks;
    const long tile = (long)(blockIdx.x / ublocks) * per + it;
    const int u0 = ub * 16 * NT;
    const int row_bytes = steps * SB;
    const __amdgpu_buffer_rsrc_t xr = dense_rows_rsrc(x, tile * 16, 16, N, row_bytes);
    const __amdgpu_buffer_rsrc_t wr = dense_rows_rsrc(wp, u0, 16 * NT, units, row_bytes);

    const int share = (steps + ks - 1) / ks;                 // this wave's K-steps: s0 .. s1 - 1, possibly none
    const int s0 = kp * share, s1 = min(s0 + share, steps);

    using Raw = decltype(dense_load<XS>(xr, 0));
    Raw ring[3][NT + 1];
    const int lane_off = r * row_bytes + h * (SB / 4);
    // a step past the share is asked for out of range: it returns zero without touching memory and is never used
    auto load = [&](Raw (&b)[NT + 1], int s) {
        const int off = lane_off + (s < s1 ? s * SB : 1 << 30);
        b[0] = dense_load<XS>(xr, off);
#pragma unroll
        for (int t = 0; t < NT; ++t) b[1 + t] = dense_load<XS>(wr, off + t * 16 * row_bytes);
    };
    v4i acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = v4i{0, 0, 0, 0};
    auto mma = [&](const Raw (&b)[NT + 1]) {
        const v4i xv = dense_operand<XS>(b[0]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(dense_operand<XS>(b[1 + t]), xv, acc[t], 0, 0, 0);
    };

    // The ring is turned by hand so that its index is a constant, three steps to a trip with no branch inside (the loads
    // keep their distance and the waits their counts); the one or two steps left over follow the loop.
    int s = s0;
    load(ring[0], s);
    load(ring[1], s + 1);
    for (; s + 3 <= s1; s += 3) {
        load(ring[2], s + 2);
        mma(ring[0]);
        load(ring[0], s + 3);
        mma(ring[1]);
        load(ring[1], s + 4);
        mma(ring[2]);
    }
    if (s < s1) mma(ring[0]);
    if (s + 1 < s1) mma(ring[1]);

    if (ks > 1) {
        if (kp > 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) meet[(((kp - 1) * per + it) * NT + t) * 64 + lane] = acc[t];
        }
        __syncthreads();
        if (kp > 0) return;
        for (int p = 0; p + 1 < ks; ++p) {
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] += meet[((p * per + it) * NT + t) * 64 + lane];
        }
    }

    const long img = tile * 16 + r;
    if (img >= N) return;
    const float scale = XS == QNN_STORE_I4 ? __fmul_rn(e.scale, 1.0f / 256.0f) : e.scale;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int u = u0 + 16 * t + 4 * h;
        if (u >= units) break;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = qnn_epi_value(__fmul_rn((float)acc[t][i], scale), u + i, e);
        const size_t at = ((size_t)img * units + u) >> 2;       // in float4s, dwords of int8 codes or half-words of int4 codes
        if constexpr (OUT == QNN_STORE_F32) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (e.fn == QNN_FN_BINARY_TANH) v[i] = qnn_binary_tanh(v[i]);
                else if (qnn_is_qact(e.fn)) v[i] = qnn_qact(e.fn, v[i], e.act_m);
            }
            ((float4*)y)[at] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            uint32_t word = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) word |= ((uint32_t)qnn_epi_code(v[i], e) & ((1u << OUT) - 1u)) << (OUT * i);
            if constexpr (OUT == QNN_STORE_I4) ((uint16_t*)y)[at] = (uint16_t)word;
            else ((uint32_t*)y)[at] = word;
        }
    }
}

// ---- launch: NT and ks from the host plan (dense_plan, qnn_dense_plan.h) --------------------------------------------
template <int XS, int OUT>
void launch_dense_mfma(const DensePlan& p, const ConvCall& c, int steps) {
    const dim3 grid(p.blocks), block(256);
    const uint8_t* x = (const uint8_t*)c.x;
    const uint8_t* wp = (const uint8_t*)c.w->d_packed;
#define DENSE_NT(NT)                                                                                                  \
    hipLaunchKernelGGL((k_dense_mfma<XS, OUT, NT>), grid, block, 0, c.s, x, wp, c.e, c.y, c.g.N, c.g.cout, steps, p.ks, \
                       p.ublocks)
    if (p.nt == 4) DENSE_NT(4);
    else if (p.nt == 2) DENSE_NT(2);
    else DENSE_NT(1);
#undef DENSE_NT
}

}  // namespace

// Takes what route_dense has declined (it stands directly behind it in kRoutes) of the dense calls on I4, I8 or BIN
// operands with cin % 64 == 0 and units % 16 == 0; the rest runs where it ran.
int qnn_route_dense_mfma(const ConvCall& c, char* name, size_t name_len) {
    const ConvGeom& g = c.g;
    const EpiArgs& e = c.e;
    const int xs = c.x_store, out = e.out_store, fn = e.fn;
    if (xs != c.w->store || (xs != QNN_STORE_I4 && xs != QNN_STORE_I8 && xs != QNN_STORE_BIN) || !c.w->d_packed) return 1;
    // cin <= 65536: K * 128 * 128 stays inside int32 with the x 16 widened int4 operands
    if (g.kh != 1 || g.kw != 1 || g.cin % 64 != 0 || g.cin > 65536 || g.cout % 16 != 0) return 1;
    if (out != QNN_STORE_F32 && out != QNN_STORE_I4 && !(out == QNN_STORE_I8 && xs != QNN_STORE_BIN)) return 1;
    // float32 output: only the layers route_dense declines for their width.  (It also declines a BIN row of kwords % 4 != 0;
    // those narrow layers stay on k_conv_ps.)
    if (out == QNN_STORE_F32 && g.cout <= 256) return 1;
    // given back after measurement (profiles/dense_mfma/README.md): at 64 images k_conv_generic's popcount loop into float32
    // takes the same 8.6 us
    if (xs == QNN_STORE_BIN && out == QNN_STORE_F32 && g.N <= 64) return 1;
    if (fn != QNN_FN_NONE && fn != QNN_FN_BINARY_TANH && !qnn_is_qact(fn)) return 1;
    if ((double)g.N * g.cout >= 2147483648.0 || (double)g.N * g.kwords >= 2147483648.0) return 1;
    DensePlan p;
    const int steps = g.cin / 64;
    if (!dense_plan(&p, g.N, g.cout, steps, 256)) return 1;          // 256 CUs
    if (xs == QNN_STORE_BIN) {
        if (out == QNN_STORE_F32) launch_dense_mfma<QNN_STORE_BIN, QNN_STORE_F32>(p, c, steps);
        else launch_dense_mfma<QNN_STORE_BIN, QNN_STORE_I4>(p, c, steps);
    } else if (xs == QNN_STORE_I4) {
        if (out == QNN_STORE_F32) launch_dense_mfma<QNN_STORE_I4, QNN_STORE_F32>(p, c, steps);
        else if (out == QNN_STORE_I4) launch_dense_mfma<QNN_STORE_I4, QNN_STORE_I4>(p, c, steps);
        else launch_dense_mfma<QNN_STORE_I4, QNN_STORE_I8>(p, c, steps);
    } else {
        if (out == QNN_STORE_F32) launch_dense_mfma<QNN_STORE_I8, QNN_STORE_F32>(p, c, steps);
        else if (out == QNN_STORE_I4) launch_dense_mfma<QNN_STORE_I8, QNN_STORE_I4>(p, c, steps);
        else launch_dense_mfma<QNN_STORE_I8, QNN_STORE_I8>(p, c, steps);
    }
    snprintf(name, name_len, "dense_mfma_%s", xs == QNN_STORE_BIN ? "bin" : xs == QNN_STORE_I4 ? "i4" : "i8");
    return 0;
}
