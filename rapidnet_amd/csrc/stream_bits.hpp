// stream_bits.hpp -- the arithmetic by which k_stream_gemv's walk (k_stream.hpp, stream_walk / stream_walk_half) reads a run of columns out of the
// column mask of the skip.  Host and device: tests/cpp/test_stream_bits.cpp checks it against a bit-by-bit loop.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RN_STREAM_BITS_HD __host__ __device__
#else
#define RN_STREAM_BITS_HD
#endif

namespace rn {

// Bits [c0, c0 + n) of the mask nz, bit 0 of the result = column c0.  nz holds 64 columns per word and ONE zero word behind the last word
// that holds a column (so the word after c0's may always be read); 1 <= n <= 64, c0 >= 0 a column of the mask.  The run may straddle two
// words; columns behind the mask's last one read as zero (the pad word and the zero tail of the last word).
RN_STREAM_BITS_HD inline unsigned long long stream_mask_bits(const unsigned long long *nz, int c0, int n) {
    const int sh = c0 & 63;
    const unsigned long long lo = nz[c0 >> 6], hi = nz[(c0 >> 6) + 1];
    unsigned long long bits = (lo >> sh) | (sh ? hi << (64 - sh) : 0ull);
    if (n < 64) bits &= (1ull << n) - 1ull;
    return bits;
}

}  // namespace rn
