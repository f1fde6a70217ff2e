// Keras' element-wise merge layers Add / Subtract / Multiply / Average / Maximum / Minimum on float32 tensors and on packed
// codes (include/qnn_abi_merge.h).  Where two low-bit branches meet, Maximum / Minimum of code tensors and Multiply of +-1 or
// ternary codes are again code tensors: the activation never exists in float32.  The other ops read the codes and write
// float32, decoding in registers.
//
// Memory-bound, no reuse, no LDS: every word is read once and written once.  One item per thread, 32-bit index arithmetic
// (the entry refuses 2^31 items or more), 64-bit tensor offsets.  The n input pointers are a kernel argument (SGPRs); the
// loop over them is unrolled over QNN_MERGE_MAX with constant indices, so the table is never indexed by a register and
// nothing goes to scratch.  The op is uniform: one scalar switch per thread in front of the body it selects.
//
//   k_merge_f32<V>            float32 -> float32.  Every input has y's shape, so the tensors are flat runs of values.
//   k_merge_codes<STORE, V>   codes -> codes of the same store and width, on whole words: OR / AND / XNOR (BIN), logic on
//                             the (mask, sign) pairs (T2), a branch-free signed maximum per field (I4 / I8): the even and the
//                             odd fields of a word are widened to bytes (I8: halves) in unsigned order, one subtraction with a
//                             guard bit per field compares all of them at once, the comparison bit is spread to a select mask.
//   k_merge_codes_f32<STORE, V>   codes -> float32: a lane owns V consecutive channels of one pixel, reads the word that
//                             holds them from every input, decodes and runs the float32 chain.
//
// V = 4 is the 16-byte form (global_load_dwordx4 / one 16-byte store per lane): every pointer 16-byte aligned and
//   f32, codes -> codes   the tensor is a flat run of whole words (no spare bits in a row's last word) of a multiple of 4
//   codes -> f32          channels a multiple of 4 (the 4 channels of a lane then share an input word)
// V = 1 is the 4-byte form for everything else: one value / one word (T2: one word pair) / one channel per lane, the spare
// bits of a row's last word masked off.
#include <stdio.h>

#include "qnn_common.h"
#include "qnn_abi_merge.h"

namespace {

constexpr int kBlock = 256;

struct MergeArgs {
    const uint32_t* x[QNN_MERGE_MAX];
    int n, op;
    uint32_t total;        // items, one per thread
    uint32_t items;        // items of one row (the forms that need the position in the row)
    uint32_t xw;           // words of one input row
    uint32_t channels;
    uint32_t tail;         // the real channels' bits in a row's last word (T2: in each plane); ~0u where the row fills it
    float scale;           // 2^-(x_bits - 1): value of one code unit (I4 / I8)
    float fn;              // (float)n, the divisor of QNN_MERGE_AVG
    FastDiv fd;            // by `items`
};

template <int W> struct Pack { uint32_t w[W]; };

template <int W>
__device__ __forceinline__ Pack<W> ld(const uint32_t* p) {
    Pack<W> r;
    if constexpr (W == 4) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        r.w[0] = v.x; r.w[1] = v.y; r.w[2] = v.z; r.w[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) r.w[j] = p[j];
    }
    return r;
}
template <int W>
__device__ __forceinline__ void st(uint32_t* p, const Pack<W>& r) {
    if constexpr (W == 4) {
        *reinterpret_cast<uint4*>(p) = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) p[j] = r.w[j];
    }
}

// ---- the float32 chain: one rounding per step; Maximum / Minimum hand a NaN on (v_max_f32 would drop it) ----------------
template <int OP>
__device__ __forceinline__ float f_step(float a, float b) {
    if constexpr (OP == QNN_MERGE_ADD || OP == QNN_MERGE_AVG) return __fadd_rn(a, b);
    else if constexpr (OP == QNN_MERGE_SUB) return __fsub_rn(a, b);
    else if constexpr (OP == QNN_MERGE_MUL) return __fmul_rn(a, b);
    else if constexpr (OP == QNN_MERGE_MAXIMUM) return a != a ? a : b != b ? b : a > b ? a : b;
    else return a != a ? a : b != b ? b : a < b ? a : b;
}
template <int OP>
__device__ __forceinline__ float f_finish(float a, float fn) {
    if constexpr (OP == QNN_MERGE_AVG) return __fdiv_rn(a, fn);
    else return a;
}

template <int V, int OP>
__device__ __forceinline__ void body_f32(uint32_t* __restrict__ y, const MergeArgs& a, uint32_t i) {
    const size_t at = (size_t)i * V;
    Pack<V> acc = ld<V>(a.x[0] + at);
#pragma unroll
    for (int k = 1; k < QNN_MERGE_MAX; ++k)
        if (k < a.n) {
            const Pack<V> v = ld<V>(a.x[k] + at);
#pragma unroll
            for (int j = 0; j < V; ++j)
                acc.w[j] = __float_as_uint(f_step<OP>(__uint_as_float(acc.w[j]), __uint_as_float(v.w[j])));
        }
#pragma unroll
    for (int j = 0; j < V; ++j) acc.w[j] = __float_as_uint(f_finish<OP>(__uint_as_float(acc.w[j]), a.fn));
    st<V>(y + at, acc);
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_merge_f32(uint32_t* __restrict__ y, const MergeArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= a.total) return;
    switch (a.op) {
        case QNN_MERGE_ADD: body_f32<V, QNN_MERGE_ADD>(y, a, i); break;
        case QNN_MERGE_SUB: body_f32<V, QNN_MERGE_SUB>(y, a, i); break;
        case QNN_MERGE_MUL: body_f32<V, QNN_MERGE_MUL>(y, a, i); break;
        case QNN_MERGE_AVG: body_f32<V, QNN_MERGE_AVG>(y, a, i); break;
        case QNN_MERGE_MAXIMUM: body_f32<V, QNN_MERGE_MAXIMUM>(y, a, i); break;
        default: body_f32<V, QNN_MERGE_MINIMUM>(y, a, i); break;
    }
}

// ---- codes -> codes --------------------------------------------------------------------------------------------------------
// One accumulator per word (T2: per word pair).  U = words it covers.
template <int STORE, int OP> struct Acc;

// BIN: the maximum of +-1 values is the OR of their bits, the minimum the AND, the product the XNOR
template <int OP> struct Acc<QNN_STORE_BIN, OP> {
    static constexpr int U = 1;
    uint32_t v;
    __device__ __forceinline__ void init(const uint32_t* w) { v = w[0]; }
    __device__ __forceinline__ void step(const uint32_t* w) {
        if constexpr (OP == QNN_MERGE_MAXIMUM) v |= w[0];
        else if constexpr (OP == QNN_MERGE_MINIMUM) v &= w[0];
        else v = ~(v ^ w[0]);
    }
    __device__ __forceinline__ void finish(uint32_t* w) const { w[0] = v; }
};

// I4 / I8: signed maximum / minimum of every field at once.  XOR with the sign bits puts the two's-complement fields in
// unsigned order; the even and the odd fields go to words of their own with an empty field above each, so
// (a | guard) - b leaves the guard bit exactly where a >= b and never borrows from the neighbour.
template <int STORE> struct Field;
template <> struct Field<QNN_STORE_I4> { static constexpr uint32_t LOW = 0x0F0F0F0Fu, GUARD = 0x10101010u, SIGN = 0x88888888u; static constexpr int SH = 4; };
template <> struct Field<QNN_STORE_I8> { static constexpr uint32_t LOW = 0x00FF00FFu, GUARD = 0x01000100u, SIGN = 0x80808080u; static constexpr int SH = 8; };

template <int STORE, int OP> struct FieldAcc {
    static constexpr int U = 1;
    typedef Field<STORE> F;
    uint32_t e, o;
    static __device__ __forceinline__ uint32_t pick(uint32_t a, uint32_t b) {
        const uint32_t ge = ((a | F::GUARD) - b) & F::GUARD;       // the guard bit of every field with a >= b
        const uint32_t m = ge - (ge >> F::SH);                     // ... spread over the field
        if constexpr (OP == QNN_MERGE_MAXIMUM) return (a & m) | (b & ~m);
        else return (b & m) | (a & ~m);
    }
    __device__ __forceinline__ void init(const uint32_t* w) {
        const uint32_t u = w[0] ^ F::SIGN;
        e = u & F::LOW;
        o = (u >> F::SH) & F::LOW;
    }
    __device__ __forceinline__ void step(const uint32_t* w) {
        const uint32_t u = w[0] ^ F::SIGN;
        e = pick(e, u & F::LOW);
        o = pick(o, (u >> F::SH) & F::LOW);
    }
    __device__ __forceinline__ void finish(uint32_t* w) const { w[0] = (e | (o << F::SH)) ^ F::SIGN; }
};
template <int OP> struct Acc<QNN_STORE_I4, OP> : FieldAcc<QNN_STORE_I4, OP> {};
template <int OP> struct Acc<QNN_STORE_I8, OP> : FieldAcc<QNN_STORE_I8, OP> {};

// T2: a (mask, sign) pair, sign = "the value is +1"; a sign bit under a clear mask bit is dropped on the way in.
// Maximum / Minimum keep the planes "is +1" and "is -1": the maximum is +1 where any input is, -1 where all are.
// Multiply keeps (mask, sign): non-zero where all are, positive where the signs agree.
template <int OP> struct Acc<QNN_STORE_T2, OP> {
    static constexpr int U = 2;
    uint32_t p, q;         // Maximum / Minimum: is +1, is -1;  Multiply: mask, sign
    __device__ __forceinline__ void init(const uint32_t* w) {
        p = OP == QNN_MERGE_MUL ? w[0] : w[1] & w[0];
        q = OP == QNN_MERGE_MUL ? w[1] & w[0] : w[0] & ~w[1];
    }
    __device__ __forceinline__ void step(const uint32_t* w) {
        if constexpr (OP == QNN_MERGE_MUL) {
            p &= w[0];
            q = ~(q ^ w[1]) & p;
        } else {
            const uint32_t pos = w[1] & w[0], neg = w[0] & ~w[1];
            if constexpr (OP == QNN_MERGE_MAXIMUM) { p |= pos; q &= neg; }
            else { p &= pos; q |= neg; }
        }
    }
    __device__ __forceinline__ void finish(uint32_t* w) const {
        w[0] = OP == QNN_MERGE_MUL ? p : p | q;
        w[1] = OP == QNN_MERGE_MUL ? q : p;
    }
};

// W words per lane: V = 4: four flat words (T2: two pairs), no spare bits anywhere; V = 1: one word (T2: one pair), the
// last one of a row masked with a.tail.
template <int STORE, int V, int OP>
__device__ __forceinline__ void body_codes(uint32_t* __restrict__ y, const MergeArgs& a, uint32_t i) {
    typedef Acc<STORE, OP> A;
    constexpr int W = V == 4 ? 4 : A::U;
    const size_t at = (size_t)i * W;
    A acc[W / A::U];
    const Pack<W> first = ld<W>(a.x[0] + at);
#pragma unroll
    for (int j = 0; j < W / A::U; ++j) acc[j].init(first.w + j * A::U);
#pragma unroll
    for (int k = 1; k < QNN_MERGE_MAX; ++k)
        if (k < a.n) {
            const Pack<W> v = ld<W>(a.x[k] + at);
#pragma unroll
            for (int j = 0; j < W / A::U; ++j) acc[j].step(v.w + j * A::U);
        }
    Pack<W> out;
#pragma unroll
    for (int j = 0; j < W / A::U; ++j) acc[j].finish(out.w + j * A::U);
    if constexpr (V == 1) {
        const uint32_t p = qnn_div(i, a.fd);
        const uint32_t keep = i - p * a.items == a.items - 1u ? a.tail : ~0u;
#pragma unroll
        for (int j = 0; j < W; ++j) out.w[j] &= keep;
    }
    st<W>(y + at, out);
}

template <int STORE, int V>
__global__ __launch_bounds__(kBlock) void k_merge_codes(uint32_t* __restrict__ y, const MergeArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= a.total) return;
    if (a.op == QNN_MERGE_MAXIMUM) body_codes<STORE, V, QNN_MERGE_MAXIMUM>(y, a, i);
    else if (a.op == QNN_MERGE_MINIMUM) body_codes<STORE, V, QNN_MERGE_MINIMUM>(y, a, i);
    else if constexpr (STORE == QNN_STORE_BIN || STORE == QNN_STORE_T2) body_codes<STORE, V, QNN_MERGE_MUL>(y, a, i);
}

// ---- codes -> float32 ------------------------------------------------------------------------------------------------------
// channel `c` (0 .. per_word - 1) of the word (T2: pair) w
template <int STORE>
__device__ __forceinline__ float decode(const uint32_t* w, int c, float scale) {
    if constexpr (STORE == QNN_STORE_BIN) {
        return ((w[0] >> c) & 1u) ? 1.0f : -1.0f;
    } else if constexpr (STORE == QNN_STORE_T2) {
        return ((w[0] >> c) & 1u) ? (((w[1] >> c) & 1u) ? 1.0f : -1.0f) : 0.0f;
    } else {
        constexpr int B = STORE == QNN_STORE_I4 ? 4 : 8;
        const int code = (int)(w[0] << (32 - B - c * B)) >> (32 - B);
        return __fmul_rn((float)code, scale);
    }
}

template <int STORE, int V, int OP>
__device__ __forceinline__ void body_codes_f32(uint32_t* __restrict__ y, const MergeArgs& a, uint32_t i) {
    constexpr int PW = STORE == QNN_STORE_I4 ? 8 : STORE == QNN_STORE_I8 ? 4 : 32;      // channels of a word (T2: pair)
    constexpr int U = STORE == QNN_STORE_T2 ? 2 : 1;
    const uint32_t p = qnn_div(i, a.fd);
    const uint32_t c0 = (i - p * a.items) * V;                     // V = 4: channels % 4 == 0, so c0 .. c0 + 3 share a word
    const size_t src = (size_t)p * a.xw + (size_t)(c0 / PW) * U;
    const int c = (int)(c0 % PW);
    Pack<V> acc;
    {
        const Pack<U> w = ld<U>(a.x[0] + src);
#pragma unroll
        for (int j = 0; j < V; ++j) acc.w[j] = __float_as_uint(decode<STORE>(w.w, c + j, a.scale));
    }
#pragma unroll
    for (int k = 1; k < QNN_MERGE_MAX; ++k)
        if (k < a.n) {
            const Pack<U> w = ld<U>(a.x[k] + src);
#pragma unroll
            for (int j = 0; j < V; ++j)
                acc.w[j] = __float_as_uint(f_step<OP>(__uint_as_float(acc.w[j]), decode<STORE>(w.w, c + j, a.scale)));
        }
#pragma unroll
    for (int j = 0; j < V; ++j) acc.w[j] = __float_as_uint(f_finish<OP>(__uint_as_float(acc.w[j]), a.fn));
    st<V>(y + (size_t)p * a.channels + c0, acc);
}

template <int STORE, int V>
__global__ __launch_bounds__(kBlock) void k_merge_codes_f32(uint32_t* __restrict__ y, const MergeArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= a.total) return;
    if (a.op == QNN_MERGE_ADD) body_codes_f32<STORE, V, QNN_MERGE_ADD>(y, a, i);
    else if (a.op == QNN_MERGE_SUB) body_codes_f32<STORE, V, QNN_MERGE_SUB>(y, a, i);
    else if (a.op == QNN_MERGE_AVG) body_codes_f32<STORE, V, QNN_MERGE_AVG>(y, a, i);
    else if constexpr (STORE == QNN_STORE_I4 || STORE == QNN_STORE_I8) body_codes_f32<STORE, V, QNN_MERGE_MUL>(y, a, i);
}

template <int V>
void launch_codes(int store, dim3 grid, hipStream_t s, uint32_t* y, const MergeArgs& a) {
    const dim3 block(kBlock);
    if (store == QNN_STORE_BIN) hipLaunchKernelGGL((k_merge_codes<QNN_STORE_BIN, V>), grid, block, 0, s, y, a);
    else if (store == QNN_STORE_I4) hipLaunchKernelGGL((k_merge_codes<QNN_STORE_I4, V>), grid, block, 0, s, y, a);
    else if (store == QNN_STORE_I8) hipLaunchKernelGGL((k_merge_codes<QNN_STORE_I8, V>), grid, block, 0, s, y, a);
    else hipLaunchKernelGGL((k_merge_codes<QNN_STORE_T2, V>), grid, block, 0, s, y, a);
}
template <int V>
void launch_codes_f32(int store, dim3 grid, hipStream_t s, uint32_t* y, const MergeArgs& a) {
    const dim3 block(kBlock);
    if (store == QNN_STORE_BIN) hipLaunchKernelGGL((k_merge_codes_f32<QNN_STORE_BIN, V>), grid, block, 0, s, y, a);
    else if (store == QNN_STORE_I4) hipLaunchKernelGGL((k_merge_codes_f32<QNN_STORE_I4, V>), grid, block, 0, s, y, a);
    else if (store == QNN_STORE_I8) hipLaunchKernelGGL((k_merge_codes_f32<QNN_STORE_I8, V>), grid, block, 0, s, y, a);
    else hipLaunchKernelGGL((k_merge_codes_f32<QNN_STORE_T2, V>), grid, block, 0, s, y, a);
}

bool merge_store_ok(int store) {
    return store == QNN_STORE_F32 || store == QNN_STORE_BIN || store == QNN_STORE_T2 || store == QNN_STORE_I4 ||
           store == QNN_STORE_I8;
}

}  // namespace

extern "C" int qnn_merge_out_store(int op, int store) {
    QNN_REQUIRE(op >= QNN_MERGE_ADD && op <= QNN_MERGE_MINIMUM, QNN_EINVAL, "qnn_merge_out_store: op=%d", op);
    QNN_REQUIRE(merge_store_ok(store), QNN_EINVAL, "qnn_merge_out_store: store=%d", store);
    if (store == QNN_STORE_F32) return QNN_STORE_F32;
    if (op == QNN_MERGE_MAXIMUM || op == QNN_MERGE_MINIMUM) return store;
    if (op == QNN_MERGE_MUL && (store == QNN_STORE_BIN || store == QNN_STORE_T2)) return store;
    return QNN_STORE_F32;
}

extern "C" int qnn_merge_forward(const qnn_merge_t* m, int store, int x_bits, size_t pixels, int channels, int out_store,
                                 void* y, void* stream) {
    const char* who = "qnn_merge_forward";
    QNN_REQUIRE(m, QNN_EINVAL, "%s: null descriptor", who);
    QNN_REQUIRE(m->n >= 2 && m->n <= QNN_MERGE_MAX, QNN_EINVAL, "%s: n=%d (2 .. %d inputs)", who, m->n, QNN_MERGE_MAX);
    QNN_REQUIRE(m->op >= QNN_MERGE_ADD && m->op <= QNN_MERGE_MINIMUM, QNN_EINVAL, "%s: op=%d", who, m->op);
    QNN_REQUIRE(m->op != QNN_MERGE_SUB || m->n == 2, QNN_EINVAL, "%s: a subtraction takes exactly 2 inputs, n=%d", who, m->n);
    QNN_REQUIRE(merge_store_ok(store), QNN_EINVAL, "%s: store=%d", who, store);
    QNN_REQUIRE(!(store == QNN_STORE_I4 || store == QNN_STORE_I8) || (x_bits >= 1 && x_bits <= store), QNN_EINVAL,
                "%s: x_bits=%d does not fit store=%d", who, x_bits, store);
    QNN_REQUIRE(channels >= 1, QNN_EINVAL, "%s: channels=%d", who, channels);
    const int want = qnn_merge_out_store(m->op, store);
    QNN_REQUIRE(out_store == want, QNN_EINVAL, "%s: out_store=%d, op=%d on store=%d gives store %d", who, out_store, m->op,
                store, want);
    const bool f32in = store == QNN_STORE_F32, f32out = out_store == QNN_STORE_F32;
    const uint64_t xw = f32in ? (uint64_t)channels : (uint64_t)qnn_words(store, channels);      // words of an input row
    const uint64_t yw = f32out ? (uint64_t)channels : xw;                                       // words of an output row
    QNN_REQUIRE(pixels < ((size_t)1 << 31) && (uint64_t)pixels * (xw > yw ? xw : yw) < ((uint64_t)1 << 31), QNN_EUNSUPPORTED,
                "%s: %zu pixels of %llu words (2^31 words or more)", who, pixels, (unsigned long long)(xw > yw ? xw : yw));
    if (pixels == 0) return QNN_OK;
    QNN_REQUIRE(y, QNN_EINVAL, "%s: y is a null pointer", who);
    const uintptr_t ya = (uintptr_t)y;
    const uint64_t ybytes = (uint64_t)pixels * yw * 4, xbytes = (uint64_t)pixels * xw * 4;
    bool aligned = ya % 16 == 0;
    for (int i = 0; i < m->n; ++i) {
        QNN_REQUIRE(m->x[i], QNN_EINVAL, "%s: x[%d] is a null pointer", who, i);
        const uintptr_t xa = (uintptr_t)m->x[i];
        QNN_REQUIRE(xa + xbytes <= ya || ya + ybytes <= xa, QNN_EINVAL, "%s: y overlaps x[%d]", who, i);
        aligned = aligned && xa % 16 == 0;
    }
    MergeArgs a;
    for (int i = 0; i < QNN_MERGE_MAX; ++i) a.x[i] = i < m->n ? (const uint32_t*)m->x[i] : nullptr;
    a.n = m->n;
    a.op = m->op;
    a.xw = (uint32_t)xw;
    a.channels = (uint32_t)channels;
    a.scale = (store == QNN_STORE_I4 || store == QNN_STORE_I8) ? 1.0f / (float)(1u << (x_bits - 1)) : 1.0f;
    a.fn = (float)m->n;
    // the real channels' bits of a row's last word (T2: of each plane of its last pair)
    const int field = f32in ? 32 : store == QNN_STORE_T2 ? 1 : 32 / qnn_per_word(store);
    const int used = (int)(((uint64_t)channels * field) % 32);
    a.tail = used == 0 ? ~0u : (1u << used) - 1u;
    const uint64_t words = (uint64_t)pixels * xw;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* yu = (uint32_t*)y;
    const char* name;
    if (f32out && !f32in) {
        const bool v4 = aligned && channels % 4 == 0;
        a.items = (uint32_t)channels / (v4 ? 4u : 1u);
        a.total = (uint32_t)(pixels * a.items);
        a.fd = qnn_fastdiv(a.items);
        const dim3 grid((a.total + kBlock - 1) / kBlock);
        if (v4) launch_codes_f32<4>(store, grid, s, yu, a);
        else launch_codes_f32<1>(store, grid, s, yu, a);
        name = store == QNN_STORE_BIN ? "merge_bin_f32" : store == QNN_STORE_I4 ? "merge_i4_f32" :
               store == QNN_STORE_I8 ? "merge_i8_f32" : "merge_t2_f32";
    } else {
        const bool v4 = aligned && a.tail == ~0u && words % 4 == 0;
        const uint32_t unit = v4 ? 4u : store == QNN_STORE_T2 ? 2u : 1u;       // words of one item
        a.items = v4 ? 1u : (uint32_t)xw / unit;                               // (V = 4 never asks for the row position)
        a.total = (uint32_t)(words / unit);
        a.fd = qnn_fastdiv(a.items);
        const dim3 grid((a.total + kBlock - 1) / kBlock), block(kBlock);
        if (f32in) {
            if (v4) hipLaunchKernelGGL((k_merge_f32<4>), grid, block, 0, s, yu, a);
            else hipLaunchKernelGGL((k_merge_f32<1>), grid, block, 0, s, yu, a);
            name = "merge_f32";
        } else {
            if (v4) launch_codes<4>(store, grid, s, yu, a);
            else launch_codes<1>(store, grid, s, yu, a);
            name = store == QNN_STORE_BIN ? "merge_bin" : store == QNN_STORE_I4 ? "merge_i4" :
                   store == QNN_STORE_I8 ? "merge_i8" : "merge_t2";
        }
    }
    QNN_HIP(hipGetLastError());
    qnn_set_kernel_name(name);
    return QNN_OK;
}
