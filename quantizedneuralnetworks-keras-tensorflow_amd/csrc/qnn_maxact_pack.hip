// quantized_maxrelu / quantized_leakymaxrelu written as packed codes (include/qnn_abi_scaled.h): pass 2 of qnn_maxact.hip as
// a pack.  The codes are those of k_maxact_apply -- the same scales from the same word through qnn_maxact_scales, the same
// per-value arithmetic through qnn_maxact_code_f (qnn_common.h) -- stored in qnn_pack_f32's layout; the consumers multiply
// their output scale by P (qnn_scaled_scale).  DUAL also writes the float32 values k_maxact_apply would write.
//
// HBM-bound streaming: per value 4 bytes read and 0.5 (I4) / 1 (I8) written, plus 4 with DUAL.  One lane produces one whole
// 32-bit output word from 8 (I4) or 4 (I8) consecutive floats, fetched with 16-byte loads; consecutive lanes own
// consecutive words, so a wave reads 2048 / 1024 contiguous bytes and writes 256.  No LDS, no scratch; word indices are
// 32-bit (the entry refuses 2^31 words or more), addresses 64-bit.
#include "qnn_common.h"

namespace {

constexpr int kBlock = 256;
constexpr unsigned kMaxBlocks = 1u << 22;      // one word per thread and trip; more words than 2^30 take a second trip

typedef float v4f __attribute__((ext_vector_type(4)));

// VEC (uniform): channels fill whole words and x (and y) are 16-byte aligned, so word wi packs the PW floats at x + wi * PW
// with no pixel decode.  Otherwise the slow form: one word per lane all the same, its (pixel, word) decoded, up to PW scalar
// loads, the fields beyond the last channel left zero.
// x and y carry no __restrict__: y == x is allowed (a lane reads the floats of its word before it writes them).
template <int FN, int STORE, bool DUAL>
__global__ __launch_bounds__(kBlock) void k_maxact_pack(const float* x, uint32_t* __restrict__ packed, float* y,
                                                        uint32_t words, int channels, int cw, int nb, bool vec,
                                                        const uint32_t* __restrict__ word) {
    constexpr int PW = STORE == QNN_STORE_I4 ? 8 : 4;
    constexpr int BITS = 32 / PW;
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    float s_in = 0.0f, s_out = 0.0f;
    const bool ok = qnn_maxact_scales(*word, nb, &s_in, &s_out);      // one scalar load per block
    const float m = __uint_as_float((uint32_t)(127 + nb - 1) << 23);
    const float qnan = __uint_as_float(0x7FC00000u);
    // code as a float (+0 for a zero); 0 for a word outside the exact range
    auto code1 = [&](float v) { return ok ? qnn_maxact_code_f(FN, v, m, s_in) : 0.0f; };
    auto val1 = [&](float c) { return ok ? __fmul_rn(c, s_out) : qnan; };
    const uint32_t stride = gridDim.x * (uint32_t)kBlock;
    for (uint32_t wi = blockIdx.x * (uint32_t)kBlock + threadIdx.x; wi < words; wi += stride) {
        uint32_t out = 0;
        if (vec) {
            const v4f* s4 = reinterpret_cast<const v4f*>(x + (size_t)wi * PW);
            v4f v[PW / 4];
#pragma unroll
            for (int j = 0; j < PW / 4; ++j) v[j] = __builtin_nontemporal_load(&s4[j]);
#pragma unroll
            for (int j = 0; j < PW / 4; ++j) {
                v4f c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    c[k] = code1(v[j][k]);
                    out |= ((uint32_t)(int)c[k] & MASK) << ((4 * j + k) * BITS);
                }
                if constexpr (DUAL) {
                    v4f* d4 = reinterpret_cast<v4f*>(y + (size_t)wi * PW);
                    __builtin_nontemporal_store((v4f){val1(c[0]), val1(c[1]), val1(c[2]), val1(c[3])}, &d4[j]);
                }
            }
        } else {
            const uint32_t p = wi / (uint32_t)cw;
            const int w = (int)(wi - p * (uint32_t)cw);
            const size_t base = (size_t)p * (size_t)channels + (size_t)w * PW;
            const int left = channels - w * PW;
#pragma unroll
            for (int j = 0; j < PW; ++j)
                if (j < left) {
                    const float c = code1(x[base + j]);
                    out |= ((uint32_t)(int)c & MASK) << (j * BITS);
                    if constexpr (DUAL) y[base + j] = val1(c);
                }
        }
        packed[wi] = out;
    }
}

template <int FN, int STORE>
void launch_pack(const float* x, void* packed, float* y, uint32_t words, int channels, int cw, int nb, bool vec,
                 const void* ws, hipStream_t s) {
    unsigned blocks = (words + kBlock - 1) / kBlock;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    if (y)
        hipLaunchKernelGGL((k_maxact_pack<FN, STORE, true>), dim3(blocks), dim3(kBlock), 0, s, x, (uint32_t*)packed, y, words,
                           channels, cw, nb, vec, (const uint32_t*)ws);
    else
        hipLaunchKernelGGL((k_maxact_pack<FN, STORE, false>), dim3(blocks), dim3(kBlock), 0, s, x, (uint32_t*)packed, y, words,
                           channels, cw, nb, vec, (const uint32_t*)ws);
}

}  // namespace

extern "C" int qnn_maxact_pack_f32(const float* x, void* packed, float* y_or_null, size_t pixels, int channels, int fn, int nb,
                                   int store, const void* workspace16, void* stream) {
    QNN_REQUIRE(qnn_is_maxact(fn), QNN_EINVAL,
                "qnn_maxact_pack_f32: fn=%d is neither QNN_FN_QUANTIZED_MAXRELU nor QNN_FN_QUANTIZED_LEAKYMAXRELU", fn);
    QNN_REQUIRE(store == QNN_STORE_I4 || store == QNN_STORE_I8, QNN_EINVAL,
                "qnn_maxact_pack_f32: store=%d is neither QNN_STORE_I4 nor QNN_STORE_I8", store);
    QNN_REQUIRE(nb >= 2 && nb <= 8 && nb <= store, QNN_EINVAL, "qnn_maxact_pack_f32: nb=%d does not fit %d-bit storage (2 .. 8)",
                nb, store);
    QNN_REQUIRE(channels > 0, QNN_EINVAL, "qnn_maxact_pack_f32: channels=%d", channels);
    if (pixels == 0) return QNN_OK;
    QNN_REQUIRE(x && packed && workspace16, QNN_EINVAL, "qnn_maxact_pack_f32: null pointer");
    const int cw = qnn_words(store, channels);
    QNN_REQUIRE((double)pixels * (double)cw < 2147483648.0, QNN_EUNSUPPORTED,
                "qnn_maxact_pack_f32: %zu pixels x %d words are 2^31 items or more in one call", pixels, cw);
    const uint32_t words = (uint32_t)(pixels * (size_t)cw);
    const bool vec = (channels % qnn_per_word(store)) == 0 && ((uintptr_t)x % 16) == 0 &&
                     (!y_or_null || ((uintptr_t)y_or_null % 16) == 0);
    hipStream_t s = (hipStream_t)stream;
    const bool leaky = fn == QNN_FN_QUANTIZED_LEAKYMAXRELU;
    if (store == QNN_STORE_I4) {
        if (leaky) launch_pack<QNN_FN_QUANTIZED_LEAKYMAXRELU, QNN_STORE_I4>(x, packed, y_or_null, words, channels, cw, nb, vec, workspace16, s);
        else launch_pack<QNN_FN_QUANTIZED_MAXRELU, QNN_STORE_I4>(x, packed, y_or_null, words, channels, cw, nb, vec, workspace16, s);
    } else {
        if (leaky) launch_pack<QNN_FN_QUANTIZED_LEAKYMAXRELU, QNN_STORE_I8>(x, packed, y_or_null, words, channels, cw, nb, vec, workspace16, s);
        else launch_pack<QNN_FN_QUANTIZED_MAXRELU, QNN_STORE_I8>(x, packed, y_or_null, words, channels, cw, nb, vec, workspace16, s);
    }
    qnn_set_kernel_name(store == QNN_STORE_I4 ? (y_or_null ? "maxact_pack_i4_dual" : "maxact_pack_i4")
                                              : (y_or_null ? "maxact_pack_i8_dual" : "maxact_pack_i8"));
    QNN_HIP(hipGetLastError());
    return QNN_OK;
}
