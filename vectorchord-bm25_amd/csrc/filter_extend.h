// filter_extend.h -- filter_extend_growing_kernel: a filter's growing bitmaps extended in place after an append.
// Included by filter.hip only (a non-template kernel: one definition).
#ifndef VBM25_FILTER_EXTEND_H
#define VBM25_FILTER_EXTEND_H

#include <hip/hip_runtime.h>
#include <cstdint>

namespace vbm25 {

// vbm25_filter_extend_growing: the delta bitmaps (F x dw words, bit j of delta i = growing document n_old + j) merged into the
// filter's growing bitmaps on the device.  One thread per (bitmap i, word w) with w0 <= w < w1: the word is what the bitmap held
// (words below old_words, from src at stride src_stride) ORed with the delta funnel-shifted left by s = n_old % 64 -- delta word
// j = w - n_old / 64 contributes its low 64 - s bits, word j - 1 its high s bits.  In place (src == dst, same stride) w0 is the
// boundary word n_old / 64 and only the tail is touched; a growth step runs it from w0 = 0 into the new buffer at the new stride,
// which re-strides all F bitmaps.  Every thread reads and writes its own word only.  delta NULL: all zero.
__global__ void __launch_bounds__(256) filter_extend_growing_kernel(const unsigned long long *src, uint32_t src_stride, uint32_t old_words,
                                                                    unsigned long long *dst, uint32_t dst_stride, uint32_t n_bitmaps,
                                                                    uint32_t n_old, const unsigned long long *delta, uint32_t dw, uint32_t w0,
                                                                    uint32_t w1) {
    const uint32_t span = w1 - w0;
    const unsigned long long total = (unsigned long long)n_bitmaps * span;
    const uint32_t bw = n_old >> 6, s = n_old & 63u;
    for (unsigned long long x = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t i = uint32_t(x / span), w = w0 + uint32_t(x % span);
        unsigned long long v = w < old_words ? src[size_t(i) * src_stride + w] : 0ull;
        if (delta && w >= bw) {
            const uint32_t j = w - bw;
            const unsigned long long *d = delta + size_t(i) * dw;
            if (j < dw) v |= d[j] << s;
            if (s && j >= 1u && j - 1u < dw) v |= d[j - 1u] >> (64u - s);
        }
        dst[size_t(i) * dst_stride + w] = v;
    }
}

}  // namespace vbm25

#endif
