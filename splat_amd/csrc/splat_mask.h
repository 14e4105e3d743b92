// splat_mask.h -- how a byte mask in the caller's memory (a selection) is read and ranked, written once for the kernels that
// walk one in 4096-byte spans: the selection's indices (splat_select.hip) and the index map of a removal (splat_compact.hip).
// Device code only.
#pragma once
#include "splat_internal.h"

namespace splat {

// ---------------------------------------------------------------------------
// The mask may start at any byte address: it is read on the 16-byte boundaries of its ADDRESS.  With
// head = address & 15, chunk c holds the mask's bytes 16 c - head .. 16 c - head + 15; thread t of workgroup g takes chunk
// 256 g + t -- one 16-byte load where the chunk lies inside the mask, byte loads of the bytes that do where it does not (the
// first chunk and the last): nothing outside mask[0..n) is read.  bits: bit k set = byte k of the chunk is nonzero.
// ---------------------------------------------------------------------------
static __device__ __forceinline__ unsigned int nonzero_bytes(unsigned int w) {     // one bit per nonzero byte of a word
    return (unsigned int)((w & 0x000000ffu) != 0u) | ((unsigned int)((w & 0x0000ff00u) != 0u) << 1) |
           ((unsigned int)((w & 0x00ff0000u) != 0u) << 2) | ((unsigned int)((w & 0xff000000u) != 0u) << 3);
}
// first: the mask index of the chunk's byte 0 (negative in the first chunk of a mask that starts off a boundary)
static __device__ __forceinline__ unsigned int chunk_bits(const unsigned char* __restrict__ mask, uint64_t n, unsigned int head,
                                                          uint64_t chunk, int64_t* first) {
    const int64_t i0 = (int64_t)(chunk * 16u) - (int64_t)head;
    *first = i0;
    if (i0 >= (int64_t)n) return 0u;
    if (i0 >= 0 && i0 + 16 <= (int64_t)n) {
        const uint4 v = *reinterpret_cast<const uint4*>(mask + i0);                 // (16-byte aligned by construction)
        return nonzero_bytes(v.x) | (nonzero_bytes(v.y) << 4) | (nonzero_bytes(v.z) << 8) | (nonzero_bytes(v.w) << 12);
    }
    unsigned int bits = 0u;
    for (int k = 0; k < 16; ++k) {
        const int64_t i = i0 + k;
        if (i >= 0 && i < (int64_t)n && mask[i] != 0) bits |= 1u << k;
    }
    return bits;
}
// Where a lane's selected bytes rank among its wave's, in index order (lane by lane, byte by byte): for each of the sixteen
// byte positions a ballot of the lanes that hold a selected byte there; those of the lanes below (mbcnt) come first.
// *total: the wave's selected bytes.
static __device__ __forceinline__ unsigned int wave_rank(unsigned int bits, unsigned int* total) {
    unsigned int rank = 0u, tot = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const unsigned long long b = __ballot((bits >> k) & 1u);
        rank += __builtin_amdgcn_mbcnt_hi((unsigned int)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)b, 0u));
        tot += (unsigned int)__popcll(b);
    }
    *total = tot;
    return rank;
}

}  // namespace splat
