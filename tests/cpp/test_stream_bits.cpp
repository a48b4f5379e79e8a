// stream_mask_bits (csrc/stream_bits.hpp) -- the run of column-mask bits a lane of k_stream_gemv's walk reads for its span or half-span --
// against a bit-by-bit loop over the same mask.  Host only: the helper is __host__ __device__ and this program compiles it with g++.
// The masks are laid out as the kernel's sh_nz: 64 columns per word, zero above column ny - 1, one zero word of padding.
// Cases: every (ny, n) with n = G or G / 2 of the spans the library chooses (1 .. 64), every unit start c0 = k * n < ny -- runs inside one
// word, runs that straddle two words, runs that end in the zero tail or reach into the pad word -- on all-ones, all-zero, single-bit and
// pseudo-random masks.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "stream_bits.hpp"

static unsigned long long naive(const std::vector<bool> &col, int c0, int n) {
    unsigned long long r = 0;
    for (int i = 0; i < n; i++)
        if (c0 + i < (int)col.size() && col[c0 + i]) r |= 1ull << i;
    return r;
}

static std::vector<unsigned long long> pack(const std::vector<bool> &col) {
    const int ny = (int)col.size();
    std::vector<unsigned long long> nz((ny + 63) / 64 + 1, 0ull);      // (the last word stays zero: the pad)
    for (int c = 0; c < ny; c++)
        if (col[c]) nz[c >> 6] |= 1ull << (c & 63);
    return nz;
}

int main() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&rng]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    long checked = 0, straddles = 0, padReads = 0;
    const int nys[] = {1, 2, 19, 63, 64, 65, 127, 128, 129, 191, 236, 240, 282, 1000};
    for (int ny : nys) {
        for (int kind = 0; kind < 6; kind++) {
            std::vector<bool> col(ny, false);
            if (kind == 0) col.assign(ny, true);
            else if (kind == 2) col[ny - 1] = true;
            else if (kind == 3) col[(ny - 1) / 2] = true;
            else if (kind >= 4) for (int c = 0; c < ny; c++) col[c] = (next() % (kind == 4 ? 2 : 10)) == 0;
            const std::vector<unsigned long long> nz = pack(col);
            for (int n = 1; n <= 64; n++)
                for (int c0 = 0; c0 < ny; c0 += n) {
                    const unsigned long long got = rn::stream_mask_bits(nz.data(), c0, n), want = naive(col, c0, n);
                    if (got != want) {
                        std::printf("FAIL ny %d kind %d n %d c0 %d: got %016llx want %016llx\n", ny, kind, n, c0, got, want);
                        return 1;
                    }
                    checked++;
                    if ((c0 & 63) + n > 64) straddles++;
                    if ((c0 >> 6) + 1 == (int)nz.size() - 1) padReads++;
                }
        }
    }
    if (straddles == 0 || padReads == 0) { std::printf("FAIL: the cases do not reach two words (%ld) or the pad word (%ld)\n", straddles, padReads); return 1; }
    std::printf("stream_mask_bits: %ld runs checked, %ld straddle two words, %ld read the pad word: all equal the bit-by-bit loop\n", checked, straddles, padReads);
    return 0;
}
