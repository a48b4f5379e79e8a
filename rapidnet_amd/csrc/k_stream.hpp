// k_stream.hpp -- the dominant kernel: all per-node mat-vecs of the backward sweep in one streaming launch (k_stream_gemv), and the structured mode's elementwise part
// (part of the kernel sources of librapidnet_hip.so; kernels.hpp includes every family header, the translation units k_*.hip instantiate them)
#pragma once
#include "common.hpp"
#include "stream_bits.hpp"

namespace rn {

// ------------------------------------------------------------------------------------------------------
// The dominant kernel.  Batched per-node mat-vec  [m1_i; m2_i] = A_i y_i  for ALL nodes of the tree in one
// launch (SmpcController.cu:617-638 issues these as 4 cublasSgemmBatched per stage inside the sequential sweep;
// they do not depend on the recursion, only the vector sums do -- see k_up_*).  One workgroup per node.
//
// Access shape (decided by measurement, tools/probe_hbm.py): a do-nothing reader with one workgroup per 376 KB node
// block reaches 6.7-6.8 TB/s on MI355X when every wave-load is 64 lanes x 16 B = 1 KB CONTIGUOUS, and only 5.9 TB/s
// when a lane fetches 32 adjacent bytes as two loads (each wave-load then touches 16 cache lines and uses half of
// each) -- which is what "4 fp64 rows per lane" amounts to.  So the block is walked in 16-byte SLOTS: a column of A_i
// (LD values) is SPC = LD*sizeof(T)/16 slots, a SPAN is G consecutive columns, and thread t owns slots t, t+512, ...
// (NL of them) of every span: consecutive threads read consecutive 16 B, across column boundaries, and each thread always
// meets the same rows, so its partial sums stay in registers.  G is chosen on the host (Ctx::stream_shape) so that a
// span is a whole number of 128-byte lines: with spans that end inside a line (first version: G = 5, 490 of 512 slots
// busy) the two wave-loads sharing that line are issued a group apart and the non-temporal stream fetches it twice --
// FETCH_SIZE showed 4.35 GB per launch against 4.09 GB algorithmic; with G = 8 (784 slots = 98 lines, NL = 2, 77 % of
// the lanes busy) it is 4.14 GB and the kernel 6 % faster.  Loads are non-temporal (A is read once per iteration and is
// far larger than the 256 MiB Infinity Cache) and double-buffered in groups of D spans (one 8-wave workgroup per CU
// with 10 x 16 B per lane in flight measured best: 512 threads, D = 5; the two-per-CU instantiation: D = 4).  Also emits a_i = F_i' xi_i (F_i is diagonal:
// Utilities.cu:33-58).
// HBM bytes per node: LD*ny*sizeof(T) + (ny + 2nv + nx)*sizeof(T).
// SPLIT = false is the kernel as it always was (span0 = 0, every block one workgroup): the instantiation the unsplit launches run --
// the whole 493-scenario tree among them, where the split gains nothing and the second code path would cost (same-box A/B against
// the round-3 kernel: 605 instead of 590 us with one shared instantiation, whose register allocation let two workgroups share a CU)
// NR = 2: TWO right-hand sides in one pass over the blocks (the quasi-Newton loops' pairs of independent Hessian sweeps: the launch is
// bound by the blocks' bytes, so the second product rides for free): the second vector r2.w, its results in r2.my / r2.qa.  Each
// right-hand side's sums are formed exactly as the one-vector kernel forms them (same order over the columns): bitwise the results
// of two launches.  Unsplit launches with w in memory only.
// THE SKIP (sp.skip != 0).  Column c of A_i only ever meets w_i[c], and most entries of an accelerated dual are exact zeros (constraints that
// were never violated: the sparse active set of the problem).  A span whose G entries of w are all +-0 adds a * (+-0) = +-0 to partial sums
// that started at +0 -- x + (+-0) = x for every x but -0, and a partial cannot become -0 from a +0 start -- so the walk leaves such spans
// out: for finite block entries the outputs are the bits of the walk over every span.  (An Inf / NaN block entry against a zero dual gave NaN
// and now gives the finite sum.)  Any bit but the sign makes an entry live: -0.0 is zero, a denormal is not.
//   While the workgroup copies w into LDS every wave ballots "entry is live" over its 64 columns into sh_nz (one word per 64 columns, one zero
// word of padding); behind the barrier every wave derives for itself, one lane per span, which spans of [span0, span1) are live: one ballot
// per chunk of 64 spans, a wave-uniform mask -- no second barrier, no list in LDS.  Groups of D LIVE spans are double-buffered as the
// groups of D consecutive spans were (scalar span index, steady state without a branch); the live count mod D is a partial group in FRONT of the
// full ones, and the ragged last span of ny % G columns, where live, a guarded load by itself behind them.  A thread keeps its slots and its rows
// and meets the live spans in increasing order.  The first group cannot be requested before
// w has arrived any more.  sp.skip == 0: every span is walked (the mask is "span exists").
// Returns what was walked: spans, columns, and whether the ragged last span was among them.
// NL = 2 (the 493-scenario tree in every precision): the unit of the skip is HALF a span and the walk is stream_walk_half, below; stream_walk is the
// walk of NL = 1, 3, 4.
__device__ __forceinline__ bool stream_nz(double v) { return ((unsigned long long)__double_as_longlong(v) << 1) != 0ull; }
__device__ __forceinline__ bool stream_nz(float v) { return (__float_as_uint(v) << 1) != 0u; }
// The multiply-add of both walks.  In the fp32 kernels it is ONE fused operation, said so here and not left to the compiler's contraction: that fused most
// of them (v_pk_fma_f32) and left some as v_pk_mul_f32 + v_pk_add_f32 -- which ones depended on the instantiation (NL = 1: 12 to 14 packed pairs per right-hand
// side, NL = 2 with two right-hand sides: one), so the same column rounded once in one instantiation and twice in another, and two right-hand sides in one pass
// were not the bits of two launches (tests/test_gpu_stream_product.py).  The fp64 sums are written as they always were -- every one of them is contracted to
// v_fma_f64 / v_fmac_f64 in every instantiation -- and those kernels' code is unchanged.
__device__ __forceinline__ double stream_fma(double a, double b, double c) { return c + a * b; }
__device__ __forceinline__ float stream_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// The group schedule of both walks.  Each walk defines RN_GROUP (its group size: D spans, or DU units), RN_POP (the next live index of the chunk's mask into sv[d]),
// RN_LOAD1 / RN_USE1 (request / consume what a thread owns of span or unit sv[d]) and the buffers bufA / bufB with their index sets sA / sB.  A chunk's nLive =
// nGroups * RN_GROUP + nHead live ones: the live count mod the group size goes FIRST (they are met in increasing order either way), as a partial group (RN_LOADH /
// RN_USEH: the first nHead, whole ones) in the second buffer, with the first full group requested right behind it: the chunk's last loads are then those of a full
// group.  The steady state has no branch inside, so the compiler's vmcnt waits are exact: while group g is consumed, group g+1 (and then g+2) is in flight.
// THE WAIT COUNTS.  A request of the partial group and its use stand under two `if (d < nHead)` that the compiler cannot pair: it sees a path on which a buffer's
// request is never waited for, carries that around the chunk loop, and in front of the next write to those registers -- the ADDRESS of a request is formed in the
// register it loads into -- it waits for everything in flight (s_waitcnt vmcnt(0)).  In the ISA of the first version every request of the partial group was thus
// issued only when the one before it had ARRIVED: one round trip per unit of the head, and with the skip a block is little more than a head (about 20 live units
// of 60: a head of 4 and two groups).  RN_LANDED(n) states what the schedule guarantees at a point -- at most the n most recent requests are
// still in flight -- as an s_waitcnt of the walk's own; it waits for nothing at run time, since what it names has been consumed: behind the partial group's use
// (only the first full group, RN_GROUP_LOADS requests, can be in flight) and at the end of a chunk (nothing is).  The compiler's counts start from there, and the
// head's requests and the first full group's go out back to back.
__host__ __device__ constexpr int stream_vmcnt(int n) { return (n & 15) | ((n >> 4) << 14) | 0x0F70; }      // gfx9 encoding of s_waitcnt: vmcnt(n), the other counters free
#define RN_LANDED(n) __builtin_amdgcn_s_waitcnt(stream_vmcnt(n));
#define RN_LOADG(buf, sv) _Pragma("unroll") for (int d = 0; d < RN_GROUP; d++) { RN_POP(sv, d) RN_LOAD1(buf, sv, d) }
#define RN_USEG(buf, sv) _Pragma("unroll") for (int d = 0; d < RN_GROUP; d++) RN_USE1(buf, sv, d)
#define RN_LOADH(buf, sv) _Pragma("unroll") for (int d = 0; d < RN_GROUP - 1; d++) if (d < nHead) { RN_POP(sv, d) RN_LOAD1(buf, sv, d) }
#define RN_USEH(buf, sv) _Pragma("unroll") for (int d = 0; d < RN_GROUP - 1; d++) if (d < nHead) RN_USE1(buf, sv, d)
#define RN_STREAM_GROUPS                                                                                               \
    RN_LOADH(bufB, sB)                                                                                                 \
    if (nGroups > 0) RN_LOADG(bufA, sA)                                                                                \
    RN_USEH(bufB, sB)                                                                                                  \
    if (nGroups > 0) {                                                                                                 \
        RN_LANDED(RN_GROUP_LOADS)                                                                                      \
        int g = 0;                                                                                                     \
        for (; g + 2 < nGroups; g += 2) {                                                                              \
            RN_LOADG(bufB, sB)                                                                                         \
            RN_USEG(bufA, sA)                                                                                          \
            RN_LOADG(bufA, sA)                                                                                         \
            RN_USEG(bufB, sB)                                                                                          \
        }                                                                                                              \
        if (g + 1 < nGroups) {                                                                                         \
            RN_LOADG(bufB, sB)                                                                                         \
            RN_USEG(bufA, sA)                                                                                          \
            RN_USEG(bufB, sB)                                                                                          \
        } else {                                                                                                       \
            RN_USEG(bufA, sA)                                                                                          \
        }                                                                                                              \
    }                                                                                                                  \
    RN_LANDED(0)
template <typename T, typename VT, int VPL, int NL, int D, int NR>
__device__ __forceinline__ void stream_walk(const VT *__restrict__ Ab, const T *sh_y, const T *sh_y2, const unsigned long long *sh_nz, int skip, int span0, int span1, int G, int ny,
                                            int spanSlots, const int (&off)[NL], const int (&cj)[NL], const T (&msk)[NL], T (&part)[NL][VPL],
                                            T (&part2)[NR == 2 ? NL : 1][VPL], int &liveSpans, int &liveCols, int &liveRagged) {
    const int lane = threadIdx.x & 63;
    const int rag = (ny % G != 0 && span1 * G > ny) ? ny / G : -1;      // the ragged last span, where this range holds it
    VT bufA[D][NL], bufB[D][NL];
    int sA[D], sB[D];
    liveSpans = 0; liveCols = 0; liveRagged = 0;
    // a load's address is (scalar) start of the span + (32-bit, per lane) byte offset of the slot: one address register per slot, whatever the span
    const char *const Abb = reinterpret_cast<const char *>(Ab);
    const unsigned spanBytes = (unsigned)spanSlots * 16u;
    unsigned offB[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) offB[j] = (unsigned)off[j] * 16u;
#define RN_POP(sv, d) { sv[d] = __builtin_amdgcn_readfirstlane(cb + __builtin_ctzll(mf)); mf &= mf - 1ull; }
#define RN_GROUP D
#define RN_GROUP_LOADS (D * NL)
#define RN_LOAD1(buf, sv, d)                                                                                           \
    _Pragma("unroll") for (int j = 0; j < NL; j++)                                                                     \
        buf[d][j] = __builtin_nontemporal_load(reinterpret_cast<const VT *>(Abb + (size_t)sv[d] * spanBytes + offB[j]));
#define RN_USE1(buf, sv, d)                                                                                            \
    _Pragma("unroll") for (int j = 0; j < NL; j++) {                                                                   \
        const T yc = sh_y[sv[d] * G + cj[j]] * msk[j];                                                                 \
        _Pragma("unroll") for (int e = 0; e < VPL; e++) part[j][e] = stream_fma((T)buf[d][j][e], yc, part[j][e]);      \
        if (NR == 2) {      /* (fp32 blocks under fp64 sums: the lane's values are converted once and meet both columns) */ \
            const T yc2 = sh_y2[sv[d] * G + cj[j]] * msk[j];                                                           \
            _Pragma("unroll") for (int e = 0; e < VPL; e++) part2[j][e] = stream_fma((T)buf[d][j][e], yc2, part2[j][e]); \
        }                                                                                                              \
    }
    for (int cb = span0; cb < span1; cb += 64) {      // chunks of 64 spans: a group never crosses a chunk
        const int s = cb + lane;
        int cols = 0;
        if (s < span1) {
            const int c0 = s * G;
            if (skip) {      // the span's G bits of the column mask (they may straddle two words)
                cols = __popcll(stream_mask_bits(sh_nz, c0, G));
            } else {
                cols = ny - c0 < G ? ny - c0 : G;
            }
        }
        const unsigned long long m = __ballot(cols > 0);
        liveSpans += __popcll(m);
        if (threadIdx.x < 64) {      // (the record: the first wave's lane 0 keeps it)
            int t = cols;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            liveCols += t;
        }
        const unsigned long long ragBit = (rag >= cb && rag < cb + 64) ? (m & (1ull << (rag - cb))) : 0ull;
        unsigned long long mf = m & ~ragBit;
        const int nLive = __popcll(mf), nGroups = nLive / D, nHead = nLive - nGroups * D;
        RN_STREAM_GROUPS
        if (ragBit) {      // the ragged last span (ny % G columns), where it is live: guarded, by itself, last
            liveRagged = 1;
            VT bufR[NL];
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const bool ok = msk[j] != (T)0 && rag * G + cj[j] < ny;      // (a column of the block: the slot lies inside it)
                bufR[j] = __builtin_nontemporal_load(reinterpret_cast<const VT *>(Abb + (size_t)rag * spanBytes + (ok ? offB[j] : 0u)));
            }
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const int c = rag * G + cj[j];
                const bool ok = msk[j] != (T)0 && c < ny;
                const T yc = ok ? sh_y[c] : (T)0;
#pragma unroll
                for (int e = 0; e < VPL; e++) part[j][e] = stream_fma((T)bufR[j][e], yc, part[j][e]);
                if (NR == 2) {
                    const T yc2 = ok ? sh_y2[c] : (T)0;
#pragma unroll
                    for (int e = 0; e < VPL; e++) part2[j][e] = stream_fma((T)bufR[j][e], yc2, part2[j][e]);
                }
            }
        }
    }
#undef RN_GROUP
#undef RN_GROUP_LOADS
#undef RN_POP
#undef RN_LOAD1
#undef RN_USE1
}
// THE WALK OVER HALF-SPANS: what every NL = 2 instantiation runs (the kernels choose it with if constexpr; stream_walk above is NL = 1, 3, 4).
// A thread's two slots of a span are two UNITS of the walk, unit u = 2 * span + h, ONE load per thread each.
//   G even (stream_slots): h is the half of the span -- unit u holds the columns [u * G/2, (u + 1) * G/2), S/2 = G/2 * SPC slots, and on the
// shapes the host admits (Ctx::stream_half_on) a whole number of 128-byte lines (fp64, 2nv = 194: 4 columns x 196 doubles = 6 272 B = 49
// lines).  Thread t' < S/2 owns slot t' of the first half and slot S/2 + t' of the second: S/2 is a multiple of SPC, so both are the thread's
// same rows.  Threads >= S/2 are idle as the padded lanes always were (a clamped address, nothing stored in sh_red), and a wave without any
// slot does not enter the walk.  With halfOn the SKIP works on units: one lane per unit reads its G/2 bits of sh_nz (stream_mask_bits).  On the
// 493-scenario tree 0.33 of the half-spans are live against 0.48 of the spans (61 % of the live spans have one live half).
//   G odd, or halfOn == 0 (RN_KNOB_STREAM_HALF = 0, halves that are not whole lines): the slots are those of the span walk where G is odd (t and
// t + 512), and both units of a span take the SPAN's liveness (each lane reads the span's G bits): the same code, the traffic of the span walk.
//   Chunks of 64 units = 32 spans; groups of 2 D live units (the requests in flight and the buffer registers of D spans x 2 loads); the partial
// group goes in front; the steady state has no branch.  h is a scalar (the popped index's low bit) and selects, by scalar-conditioned moves,
// the slot's offset and column and which accumulator meets the dual entry -- the other one meets +0: a * (+0) added to a partial that began at
// +0 changes no bit, for the reason the skip changes none (and like the skip it presumes finite block entries).  Every slot's partial still
// meets its spans in increasing order: the outputs are the bits of the span walk and of the walk over everything.
//   The ragged last span: each of its live units a guarded load of its own behind the groups.  span0 / span1, liveSpans, liveCols and liveRagged
// are in SPANS as in stream_walk; liveUnits counts the units walked (bits 0-15; with halfOn the live units of the ragged span among them in bits
// 16-19 and their columns from bit 20 on: rn_algorithmic_bytes counts those units at the columns they have).
template <typename T, typename VT, int VPL, int DU, int NR>
__device__ __forceinline__ void stream_walk_half(const VT *__restrict__ Ab, const T *sh_y, const T *sh_y2, const unsigned long long *sh_nz, int skip, int halfOn, int span0, int span1,
                                                 int G, int ny, int spanSlots, const int (&off)[2], const int (&cj)[2], const T (&msk)[2], T (&part)[2][VPL],
                                                 T (&part2)[NR == 2 ? 2 : 1][VPL], int &liveSpans, int &liveCols, int &liveRagged, int &liveUnits) {
    const int lane = threadIdx.x & 63, Gh = G >> 1;
    const int u0 = 2 * span0, u1 = 2 * span1;
    const int rag = (ny % G != 0 && span1 * G > ny) ? ny / G : -1;      // the ragged last span, where this range holds it
    VT bufA[DU], bufB[DU];
    int sA[DU], sB[DU];
    liveSpans = 0; liveCols = 0; liveRagged = 0; liveUnits = 0;
    const char *const Abb = reinterpret_cast<const char *>(Ab);
    const unsigned spanBytes = (unsigned)spanSlots * 16u;
    const unsigned offB[2] = {(unsigned)off[0] * 16u, (unsigned)off[1] * 16u};
#define RN_GROUP DU
#define RN_GROUP_LOADS DU
#define RN_POP(sv, d) { sv[d] = __builtin_amdgcn_readfirstlane(ub + __builtin_ctzll(mf)); mf &= mf - 1ull; }
#define RN_LOAD1(buf, sv, d) buf[d] = __builtin_nontemporal_load(reinterpret_cast<const VT *>(Abb + (size_t)(sv[d] >> 1) * spanBytes + ((sv[d] & 1) ? offB[1] : offB[0])));
#define RN_USE1(buf, sv, d) {                                                                                          \
        const bool h1 = (sv[d] & 1) != 0;                                                                              \
        const int cy = (sv[d] >> 1) * G + (h1 ? cj[1] : cj[0]);                                                        \
        const T yv = sh_y[cy];                                                                                         \
        const T ya = h1 ? (T)0 : yv, yb = h1 ? yv : (T)0;                                                              \
        _Pragma("unroll") for (int e = 0; e < VPL; e++) { part[0][e] = stream_fma((T)buf[d][e], ya, part[0][e]); part[1][e] = stream_fma((T)buf[d][e], yb, part[1][e]); } \
        if (NR == 2) {                                                                                                 \
            const T yv2 = sh_y2[cy];                                                                                   \
            const T ya2 = h1 ? (T)0 : yv2, yb2 = h1 ? yv2 : (T)0;                                                      \
            _Pragma("unroll") for (int e = 0; e < VPL; e++) { part2[0][e] = stream_fma((T)buf[d][e], ya2, part2[0][e]); part2[NR == 2 ? 1 : 0][e] = stream_fma((T)buf[d][e], yb2, part2[NR == 2 ? 1 : 0][e]); } \
        }                                                                                                              \
    }
    for (int ub = u0; ub < u1; ub += 64) {      // chunks of 64 units (ub is even: a span's two units share a chunk); a group never crosses a chunk
        const int u = ub + lane;
        // the run of columns whose liveness is the unit's: its own half, or its span
        const int c0 = halfOn ? u * Gh : (u >> 1) * G, n = halfOn ? Gh : G;
        int cols = 0;
        if (u < u1 && c0 < ny) cols = skip ? __popcll(stream_mask_bits(sh_nz, c0, n)) : (ny - c0 < n ? ny - c0 : n);
        const unsigned long long m = __ballot(cols > 0);
        liveSpans += __popcll((m | (m >> 1)) & 0x5555555555555555ull);
        liveUnits += __popcll(m);
        if (threadIdx.x < 64) {      // (the record: the first wave's lane 0 keeps it; a span's columns are counted once)
            int t = (halfOn || !(lane & 1)) ? cols : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            liveCols += t;
        }
        const int ragSh = 2 * rag - ub;
        const unsigned long long ragBits = (ragSh >= 0 && ragSh < 64) ? (m & (3ull << ragSh)) : 0ull;
        unsigned long long mf = m & ~ragBits;
        const int nLive = __popcll(mf), nGroups = nLive / DU, nHead = nLive - nGroups * DU;
        RN_STREAM_GROUPS
        if (ragBits) {      // the ragged last span: its live units, each a guarded load, last (an idle slot or one behind the block reads the block's first slot against zero)
            liveRagged = 1;
#pragma unroll
            for (int h = 0; h < 2; h++)
                if ((ragBits >> (ragSh + h)) & 1ull) {
                    if (halfOn) { const int left = ny - (2 * rag + h) * Gh; liveUnits += (1 << 16) + ((left < Gh ? left : Gh) << 20); }      // (the record: see below)
                    const int c = rag * G + cj[h];
                    const bool ok = msk[h] != (T)0 && c < ny;      // (a column of the block: the slot lies inside it)
                    const VT bufR = __builtin_nontemporal_load(reinterpret_cast<const VT *>(Abb + (ok ? (size_t)rag * spanBytes + offB[h] : (size_t)0)));
                    const T yc = ok ? sh_y[c] : (T)0;
#pragma unroll
                    for (int e = 0; e < VPL; e++) part[h][e] = stream_fma((T)bufR[e], yc, part[h][e]);
                    if (NR == 2) {
                        const T yc2 = ok ? sh_y2[c] : (T)0;
#pragma unroll
                        for (int e = 0; e < VPL; e++) part2[NR == 2 ? h : 0][e] = stream_fma((T)bufR[e], yc2, part2[NR == 2 ? h : 0][e]);
                    }
                }
        }
    }
#undef RN_GROUP
#undef RN_GROUP_LOADS
#undef RN_POP
#undef RN_LOAD1
#undef RN_USE1
#undef RN_LOADG
#undef RN_USEG
#undef RN_LOADH
#undef RN_USEH
#undef RN_STREAM_GROUPS
#undef RN_LANDED
}
// Which slots of a span thread `tid` owns: off[j] (clamped to a slot of the span for idle threads), their columns cj[j] inside the span, msk[j] = 1
// for an owned slot.  Slots tid, tid + 512, ...; NL = 2 with an even G: slot tid of each HALF of the span (stream_walk_half).
template <typename T, int NL>
__device__ __forceinline__ void stream_slots(int tid, int G, int SPC, int spanSlots, int (&off)[NL], int (&cj)[NL], T (&msk)[NL]) {
    const bool halves = NL == 2 && !(G & 1);
    const int stride = halves ? spanSlots >> 1 : STREAM_THREADS;
#pragma unroll
    for (int j = 0; j < NL; j++) {
        const int q = tid + stride * j;
        const bool ok = halves ? tid < stride : q < spanSlots;
        off[j] = ok ? q : (halves ? stride * (j + 1) - 1 : spanSlots - 1);          // idle slots re-read a last slot and are not stored
        cj[j] = off[j] / SPC;
        msk[j] = ok ? (T)1 : (T)0;
    }
}
// the NL = 2 kernels' call of the walk over units: every wave that owns a slot (the kernels call stream_walk themselves for NL = 1, 3, 4 -- through
// a common wrapper those instantiations came out of the compiler with up to 10 more VGPRs and a wave less per SIMD)
template <typename T, typename VT, int VPL, int DU, int NR>
__device__ __forceinline__ void stream_walk_two(const VT *__restrict__ Ab, const T *sh_y, const T *sh_y2, const unsigned long long *sh_nz, int skip, int halfOn, int span0, int span1,
                                                int G, int ny, int spanSlots, const int (&off)[2], const int (&cj)[2], const T (&msk)[2],
                                                T (&part)[2][VPL], T (&part2)[NR == 2 ? 2 : 1][VPL], int &liveSpans, int &liveCols, int &liveRagged, int &liveUnits) {
    liveSpans = 0; liveCols = 0; liveRagged = 0; liveUnits = 0;
    const int firstIdle = (G & 1) ? STREAM_THREADS : spanSlots >> 1;      // the first thread without a slot
    if (__builtin_amdgcn_readfirstlane((int)threadIdx.x & ~63) < firstIdle)
        stream_walk_half<T, VT, VPL, DU, NR>(Ab, sh_y, sh_y2, sh_nz, skip, (G & 1) ? 0 : halfOn, span0, span1, G, ny, spanSlots, off, cj, msk, part, part2,
                                            liveSpans, liveCols, liveRagged, liveUnits);
}
// the workgroup's copy of w (and of the second right-hand side) into LDS, and the column mask sh_nz of the skip beside it: every wave ballots its
// 64 columns (trip count the same for every thread: (ny + 63) / 64 + 1 words, the last one zero).  w0 / w20: the first STREAM_THREADS entries,
// requested by the caller in front of everything else.
template <typename T, int NR>
__device__ __forceinline__ void stream_stage_w(const T *__restrict__ w, const T *__restrict__ w2, T w0, T w20, T *sh_y, T *sh_y2, unsigned long long *sh_nz, int ny) {
    const int tid = threadIdx.x, nzWords = (ny + 63) / 64 + 1;
    for (int c0 = 0; (c0 >> 6) < nzWords; c0 += STREAM_THREADS) {
        const int c = c0 + tid;
        T v = 0, v2 = 0;
        if (c < ny) {
            v = c0 == 0 ? w0 : w[c];
            sh_y[c] = v;
            if (NR == 2) { v2 = c0 == 0 ? w20 : w2[c]; sh_y2[c] = v2; }
        }
        const unsigned long long b = __ballot(stream_nz(v) || (NR == 2 && stream_nz(v2)));
        if ((tid & 63) == 0 && (c >> 6) < nzWords) sh_nz[c >> 6] = b;
    }
}
// what a workgroup walked, for rn_debug_stream_live / rn_algorithmic_bytes (spans) and rn_debug_stream_units (the units of the walk: half-spans where
// stream_walk_half ran, i.e. NL = 2): one 8-byte and there one 4-byte store per workgroup, overwritten by every launch
template <bool UNITS>      // (the instantiations that walk spans store what they always stored: their units are the spans)
__device__ __forceinline__ void stream_record(int2 *live, int *units, int liveSpans, int liveCols, int liveRagged, int liveUnits) {
    if (threadIdx.x == 0 && live) {
        live[blockIdx.x] = make_int2(liveSpans, liveCols | (liveRagged << 30));
        if (UNITS) units[blockIdx.x] = liveUnits;
    }
}
template <typename T>
struct StreamRhs2 { const T *w; T *my; T *qa; };
// Spans per group (D, stream_walk) and units per group (DU, stream_walk_half: NL = 2) of k_stream_gemv<T, NL, SPLIT, NR, ST>.  D0 is the measured depth; the
// SPLIT instantiations with NL <= 2 walk groups one span shorter, which is what fits two workgroups per CU.  Two right-hand sides double the accumulators,
// and a group is shortened where they would not fit the registers -- by a DIFFERENT rule for each storage (the order in which a thread meets its columns
// does not depend on the depth: same sums, bit for bit).  Blocks in the context's own type, fp32 (4 values per slot x 2 accumulator sets): a group one span
// shorter (NL = 4: one span per group), 150-172 VGPRs instead of 256 + 20-28 bytes of scratch per lane with the full depth; NL = 2 one UNIT fewer (169 VGPRs
// with 8, one over what leaves three waves per SIMD as the span walk's 142 did); fp64 pairs keep the full depth.  fp32 blocks under fp64 sums: NL >= 3 runs
// groups one span shorter (NL = 4: one span per group) to stay inside the registers; NL <= 2 keeps the full depth, two units per span.
template <typename T, typename ST, int NL, bool SPLIT, int NR>
struct StreamDepth {
    static constexpr bool native = sizeof(ST) == sizeof(T);
    static constexpr bool shortPair = NR == 2 && (native ? sizeof(T) == 4 : NL >= 3);
    static constexpr int D0 = NL <= 2 ? (SPLIT ? RN_STREAM_D - 1 : RN_STREAM_D) : RN_STREAM_D_WIDE;
    static constexpr int D = shortPair ? (NL == 4 ? 1 : D0 - 1) : D0;
    static constexpr int DU = 2 * D - ((native && shortPair) ? 1 : 0);
};
// ST: the type the blocks are STORED in -- T, or float under T = double (rn_set_operator_storage(RN_STORE_F32)): half the bytes of the
// only large thing in HBM, every sum still formed in fp64.  a.A points at floats then: a.LD is 2nv rounded up to four floats, a.strideA counts floats (whole
// lines of 32), G and NL are the host's choice for 4-byte elements (Ctx::stream_shape) -- the block is walked exactly as the fp32 context walks its own
// (slots of FOUR floats, same G, same column order).  Behind the load the lane converts its floats (exact, once for both right-hand sides) and accumulates in
// double against the double sh_y; LDS sets, fold and outputs are T and go where ST = T puts them, so no consumer knows about the storage.  NR = 2 over fp32
// storage is behind rn_set_sweep_pairing(RN_PAIR_ON) (Ctx::stream_pair_ok); not measured on an MI355X yet.
// LDS: NR * (ny + G * LD) values of T (fp32 storage, NR = 2: up to the CU's 160 KB, Ctx::launch_stream).  HBM bytes per node, fp32 storage: LD*ny*4 + NR*(ny + 2nv + nx)*8.
// Registers with fp32 storage (hipcc's resource report, SPLIT = false | true; NL = 2 with the walk over half-spans, the others with the walk over live spans): NL = 1:
// 120 | 64 VGPRs, NL = 2: 211 | 125 (span walk: 184 | 156), NL = 3: 193 | 188, NL = 4: 255 | 248; no scratch (ST = T = float, NL = 2: 129 | 125 with stream_fma, double: 123 | 125 -- span
// walk 160 | 122 and 147 | 123).  NR = 2 (SPLIT = false): NL = 1: 138, NL = 2: 247 (span walk: 215), NL = 3: 210, NL = 4: 229 (groups of one span); no scratch, two waves
// per SIMD from NL = 2 on.
template <typename T, int NL, bool SPLIT, int NR = 1, typename ST = T>
__global__ void __launch_bounds__(STREAM_THREADS, RN_STREAM_MINW) k_stream_gemv(SweepArgs<T> a, int G, int node0, StreamSplit<T> sp, StreamRhs2<T> r2) {
    static_assert(NR == 1 || !SPLIT, "two right-hand sides: unsplit launches only");
    static_assert(sizeof(ST) == sizeof(T) || (sizeof(T) == 8 && sizeof(ST) == 4), "blocks are stored in the context's type, or in fp32 under fp64");
    typedef typename Slot<ST>::type VT;
    typedef StreamDepth<T, ST, NL, SPLIT, NR> Depth;
    constexpr int VPL = Slot<ST>::N, D = Depth::D, DU = Depth::DU;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *sh_y = reinterpret_cast<T *>(smem_raw);          // ny (+ G of zero padding is not needed: guarded reads)
    T *sh_red = sh_y + ((a.ny + 3) & ~3);               // G * LD
    T *sh_y2 = sh_red + (size_t)G * a.LD;               // NR = 2: the same pair again for the second right-hand side
    T *sh_red2 = sh_y2 + ((a.ny + 3) & ~3);
    const int tid = threadIdx.x;
    // blocks [0, first): one workgroup each; from there on two workgroups per block (first half, second half)
    const bool split = SPLIT && (int)blockIdx.x >= sp.first;
    const int node = split ? sp.first + (((int)blockIdx.x - sp.first) >> 1) : (int)blockIdx.x;
    const bool second = split && ((((int)blockIdx.x - sp.first) & 1) != 0);
    const int nx = a.nx, nv = a.nv, ny = a.ny, LD = a.LD;
    const int SPC = LD / VPL, spanSlots = G * SPC;
    const VT *__restrict__ Ab = reinterpret_cast<const VT *>(reinterpret_cast<const ST *>(a.A) + (size_t)node * a.strideA);
    // this workgroup's spans: [span0, span1) of the block's ceil(ny / G)
    const int spansAll = (ny + G - 1) / G;
    const int span0 = SPLIT ? (second ? sp.spanHalf : 0) : 0, span1 = (split && !second) ? sp.spanHalf : spansAll;
    int off[NL], cj[NL];
    T msk[NL];
    stream_slots<T, NL>(tid, G, SPC, spanSlots, off, cj, msk);
    T part[NL][VPL], part2[NR == 2 ? NL : 1][VPL];
#pragma unroll
    for (int j = 0; j < NL; j++)
#pragma unroll
        for (int e = 0; e < VPL; e++) { part[j][e] = 0; if (NR == 2) part2[j][e] = 0; }
    // Prologue.  A wave's loads return in order, so everything the prologue needs is requested first; the blocks' first group follows once w has
    // said which spans are live (stream_walk).
    const bool has0 = tid < ny;
    const size_t i0 = (size_t)node * ny + (has0 ? tid : 0);
    // stage of the node by arithmetic in the chain region (every stage >= chainStage has K nodes: no table load in front of
    // the preconditioner row's address); a table load for the few crown nodes before it
    const int stage = node >= node0 ? a.chainStage + (node - node0) / a.K : a.tr.stageOf[node];
    const T *dyRow = a.tr.dy + (size_t)stage * ny;
    const T spn = a.tr.sqrtp[node];
    const int tq = tid < nx ? tid : 0;
    const T dq0 = dyRow[tq], dq1 = dyRow[nx + tq];    // for a_i below
    const T w0a = a.w[i0];      // the y column: the accelerated dual the sweep is evaluated at
    T w20 = 0;
    if (NR == 2) w20 = r2.w[i0];
    // a_i is STORED AT THE END of the kernel: stores count in the same in-order counter as the loads, so a store issued
    // here has to be acknowledged before the wave may consume any group of A_i requested after it
    T qa0 = 0, qa02 = 0;
    unsigned long long *sh_nz = reinterpret_cast<unsigned long long *>(sh_y + (size_t)NR * (((ny + 3) & ~3) + (size_t)G * LD));   // (ny + 63) / 64 + 1 words
    stream_stage_w<T, NR>(a.w + (size_t)node * ny, NR == 2 ? r2.w + (size_t)node * ny : nullptr, w0a, w20, sh_y, sh_y2, sh_nz, ny);
    __syncthreads();
    // a_i = F_i' xi_i = sqrt(p_i) (d_x o xi_box + d_xs o xi_safe)      (a split block: written by its first half)
    if (tid < nx) qa0 = stream_qa_elem(spn, dq0, sh_y[tid], dq1, sh_y[nx + tid]);
    if (!second) for (int t = tid + STREAM_THREADS; t < nx; t += STREAM_THREADS)
        a.qa[(size_t)node * nx + t] = stream_qa_elem(spn, dyRow[t], sh_y[t], dyRow[nx + t], sh_y[nx + t]);
    if (NR == 2) {
        if (tid < nx) qa02 = stream_qa_elem(spn, dq0, sh_y2[tid], dq1, sh_y2[nx + tid]);
        for (int t = tid + STREAM_THREADS; t < nx; t += STREAM_THREADS)
            r2.qa[(size_t)node * nx + t] = stream_qa_elem(spn, dyRow[t], sh_y2[t], dyRow[nx + t], sh_y2[nx + t]);
    }
    int liveSpans, liveCols, liveRagged, liveUnits;
    if constexpr (NL == 2) stream_walk_two<T, VT, VPL, DU, NR>(Ab, sh_y, sh_y2, sh_nz, sp.skip, sp.half, span0, span1, G, ny, spanSlots, off, cj, msk, part, part2, liveSpans, liveCols, liveRagged, liveUnits);
    else { stream_walk<T, VT, VPL, NL, D, NR>(Ab, sh_y, sh_y2, sh_nz, sp.skip, span0, span1, G, ny, spanSlots, off, cj, msk, part, part2, liveSpans, liveCols, liveRagged); liveUnits = 0; }
#pragma unroll
    for (int j = 0; j < NL; j++)
        if (msk[j] != (T)0) {
#pragma unroll
            for (int e = 0; e < VPL; e++) { sh_red[(size_t)off[j] * VPL + e] = part[j][e]; if (NR == 2) sh_red2[(size_t)off[j] * VPL + e] = part2[j][e]; }
        }
    if (tid < nx && !second) stream_out(qa0, a.qa + (size_t)node * nx + tid);
    if (NR == 2 && tid < nx) stream_out(qa02, r2.qa + (size_t)node * nx + tid);
    stream_record<NL == 2>(sp.live, sp.units, liveSpans, liveCols, liveRagged, liveUnits);
    __syncthreads();
    T *const myOut = second ? sp.my2 + (size_t)(node - sp.first) * 2 * nv : a.my + (size_t)node * 2 * nv;
    if (NR == 2) {      // both right-hand sides' partials folded in one walk (each in the order of the one-vector kernel): the LDS round trips overlap
        T *const myOut2 = r2.my + (size_t)node * 2 * nv;
        for (int r = tid; r < 2 * nv; r += STREAM_THREADS) {
            T s = sh_red[r], s2 = sh_red2[r];
            for (int k = 1; k < G; k++) { s += sh_red[(size_t)k * LD + r]; s2 += sh_red2[(size_t)k * LD + r]; }
            stream_out(s, myOut + r);
            stream_out(s2, myOut2 + r);
        }
        return;
    }
    for (int r = tid; r < 2 * nv; r += STREAM_THREADS) {    // slot q of a span = column q / SPC, rows (q % SPC) * VPL ...
        T s = sh_red[r];
        for (int k = 1; k < G; k++) s += sh_red[(size_t)k * LD + r];
        stream_out(s, myOut + r);
    }
}

// ------------------------------------------------------------------------------------------------------
// Structured operator mode ("shared-operator model"): every per-node block of the factor step
// is (shared matrix) x (stage diagonal) x (power of p_i)  --  D_i = Bbt F_i', Ftil_i = L' G_i', Phi_i = -Omega_i D_i / 2,
// Psi_i = -Omega_i Ftil_i / 2 (Engine.cu:721-745) with F_i, G_i diagonal (Utilities.cu:33-58).  Hence
//   m2_i = D_i xi_i + Ftil_i psi_i = [Bbt | L'] [a_i; b_i],   a_i = F_i' xi_i,  b_i = G_i' psi_i     (elementwise + one GEMM)
//   m1_i = -Rinv m2_i / (2 p_i)   is folded into  v_i = -(Rinv rho_i + Rinv Bbt kappa_i) / (2 p_i)
// and no per-node block is ever stored or read.  This kernel is the elementwise part.
template <typename T>
__global__ void k_struct_prep(SweepArgs<T> a) {
    const int nx = a.nx, nu = a.nu, ny = a.ny, w = nx + nu;
    const long long n = (long long)a.nodes * w;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int node = (int)(i / w), t = (int)(i % w);
        const T *dy = a.tr.dy + (size_t)a.tr.stageOf[node] * ny;
        const size_t y = (size_t)node * ny;
        const T sp = a.tr.sqrtp[node];
        T val;
        if (t < nx) { val = sp * (dy[t] * a.w[y + t] + dy[nx + t] * a.w[y + nx + t]); a.qa[(size_t)node * nx + t] = val; }
        else { const int j = t - nx; val = sp * dy[2 * nx + j] * a.w[y + 2 * nx + j]; }
        a.ab[i] = val;
    }
}


}  // namespace rn
