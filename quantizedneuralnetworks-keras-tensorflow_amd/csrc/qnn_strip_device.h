// Device half of the walk of the row-walking strip kernels (qnn_mfma_strip.hip, qnn_mfma_strip_dil.hip,
// qnn_mfma_strip_i8.hip, qnn_mfma_strip16.hip): what a wave does once (block map, k-block table, filter load) and what it
// does once per task (task decode, image descriptors), plus the int4 widening.  The host half is qnn_strip_plan.h.
// Which kernel uses which helper, and why not every kernel uses all: profiles/strip_chain/README.md.
#pragma once
#include "qnn_mfma_common.h"

namespace {

// Workgroup -> (task stream, channel block) when a layer's channel blocks are separate workgroups (gridDim.y > 1): the
// blocks of one task stream are placed on ONE XCD (workgroups are dealt to the eight XCDs round robin in dispatch order)
// and start together, so the pieces of a stored pixel written by different blocks meet in the same L2 instead of leaving
// partial sectors in several (measured on the un-pooled int8 first layer, qnn_first_u8.hip: 0.49 -> 0.39 ms).
__device__ __forceinline__ void strip_block_map(int& xw, int& yblk) {
    xw = blockIdx.x; yblk = blockIdx.y;
    const int nsl = gridDim.y, bxw = gridDim.x;
    if (nsl > 1 && (bxw & 7) == 0) {
        const int bid = blockIdx.y * bxw + blockIdx.x;
        const int xcd = bid & 7, j = bid >> 3;
        yblk = j % nsl;
        xw = (j / nsl) * 8 + xcd;
    }
}

// The lane's 16-channel k-block in every K-step of an input row (stride 1, dilated or not): block j = 4 * st + kq is
// (tap dx = j / BP, channel group hb = j % BP), BP = CIN / 16; blocks beyond the 3 * BP of a row are not ok (zero filter).
template <int CIN, int ST>
__device__ __forceinline__ void strip_kblocks(int kq, int (&dxs)[ST], int (&hbs)[ST], bool (&kok)[ST]) {
    constexpr int BP = CIN / 16;
    static_assert(ST == (3 * BP + 3) / 4, "K-steps per input row");
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        const int j = 4 * st + kq;
        kok[st] = j < 3 * BP;
        dxs[st] = kok[st] ? j / BP : 1;
        hbs[st] = kok[st] ? j % BP : 0;
    }
}

// The stride-2 table: lane group kq owns tap dx = kq (kq = 3: zero filter), K-step st is channel group st.
template <int ST>
__device__ __forceinline__ void strip_kblocks_s2(int kq, int (&dxs)[ST], int (&hbs)[ST], bool (&kok)[ST]) {
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        kok[st] = kq < 3;
        dxs[st] = kok[st] ? kq : 1;
        hbs[st] = st;
    }
}

// Filters as the A operand, from the [cout][tap][CIN] byte image: row r of tile nt is channel nbase + 4*NT*(r>>2) + 4*nt +
// (r&3), so that a lane's 4 * NT results in the C/D layout are CONSECUTIVE channels (nbase + 4*NT*kq + 4*nt + i).
template <int CIN, int ST, int NT>
__device__ __forceinline__ void strip_load_filters(v4i (&bw)[3][ST][NT], const uint8_t* wq8, uint32_t w_bytes, int nbase,
                                                   int r, const bool (&kok)[ST], const int (&dxs)[ST], const int (&hbs)[ST]) {
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(wq8), 0, (int)w_bytes, 0x00020000);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int st = 0; st < ST; ++st)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int ch = nbase + 4 * NT * (r >> 2) + 4 * nt + (r & 3);
                const int woff = kok[st] ? (ch * 9 + dy * 3 + dxs[st]) * CIN + hbs[st] * 16 : (int)0x80000000;
                bw[dy][st][nt] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, woff, 0, 0));
            }
}

// task = (image n, strip starting at column xs, rows y0 .. y1 - 1 of the walk's `rows`): scalar decode of the plan of
// qnn_strip_plan.h, once per ~rc rows
struct StripTask {
    int n, xs, y0, y1;
};
__device__ __forceinline__ StripTask strip_task(int task, FastDiv fd_nch, int nch, FastDiv fd_spr, int spr, int rc, int rows) {
    const uint32_t rest = qnn_div((uint32_t)task, fd_nch);
    const int chunk = task - (int)rest * nch;
    const int n = (int)qnn_div(rest, fd_spr);
    const int y0 = chunk * rc;
    return StripTask{n, ((int)rest - n * spr) * 16, y0, min(y0 + rc, rows)};
}

// Buffer descriptor of ONE image of a tensor: whatever lies above, below or beside it is out of range (loads return 0,
// stores are dropped), which is all the zero padding and edge handling the walks have.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t strip_image_rsrc(const void* base, int n, uint32_t img_bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((uint8_t*)const_cast<void*>(base) + (size_t)n * img_bytes, 0, (int)img_bytes, 0x00020000);
}

// sixteen int4 codes -> code * 16 bytes, the int8 operand of the MFMA (x256 is folded into the output scale)
__device__ __forceinline__ v4i strip_widen(const uint2& q) {
    const uint4 v = make_uint4((q.x << 4) & 0xF0F0F0F0u, q.x & 0xF0F0F0F0u, (q.y << 4) & 0xF0F0F0F0u, q.y & 0xF0F0F0F0u);
    return __builtin_bit_cast(v4i, v);
}

}  // namespace
