// Ordered stream compaction in three passes, the one copy.  Users: cloud.hip (the set mask pixels), cloud_eval.hip (the heads of the sorted cell
// keys; the undecided points of a thinning round) and mesh.hip (the extraction's vertex and face slots, the selection's vertices and faces, the
// heads of the sorted edge keys).
// count: a 256-thread block walks a tile of TILE positions - wave v owns positions [v, v + 1) * TILE / 4 in ITER = TILE / 256 rows of 64, one
// ballot per row - and writes one partial; scan: ONE block turns the partials into 64-bit exclusive offsets; emit: the ballots again, and a
// set position goes to offsets[block] + the totals of the block's earlier waves + the set bits of the wave's earlier rows + its lane rank.
// The output order is the position order and a pure function of the flags: no atomics, no output cursor, the same bytes on every run.
//
// Which form to reach for: a kernel is its predicate, its addresses and one call - compact_count in the count kernel, compact_emit with the
// body of a set position in the emit kernel, compact_scan in a scan kernel of the caller's own (what follows the scan differs per caller).
// The pieces underneath (compact_ballots, compact_block_total, compact_wave_base, compact_rank) are for a kernel that does more in the row
// loop than emit set positions; grid_emit_kernel (cloud_eval.hip) is the one that does: it also writes cell_start[ncells] from a position that
// need not be set.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned compact_rank(unsigned long long ballot) {   // set lanes below this one
    return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// first position of this lane in the block's tile (Pos: the caller's position type); its row j is at + 64 * j
template <int TILE, typename Pos>
__device__ __forceinline__ Pos compact_seg() {
    return (Pos)blockIdx.x * (Pos)TILE + (threadIdx.x >> 6) * (TILE / 4) + (threadIdx.x & 63);
}

// tile walk: bal[j] = ballot of set(seg + 64 * j); returns the wave's total (the count pass never reads its bal[]: it costs no register)
template <int ITER, typename Pos, typename Set>
__device__ __forceinline__ unsigned compact_ballots(Pos seg, Set set, unsigned long long (&bal)[ITER]) {
    unsigned tot = 0;
#pragma unroll
    for (int j = 0; j < ITER; ++j) {
        bal[j] = __ballot(set(seg + 64 * j));
        tot += (unsigned)__popcll(bal[j]);
    }
    return tot;
}

// count pass: the block's total from the four wave totals (16 B of LDS, one barrier); uniform, only thread 0 stores it: no guard needed
__device__ __forceinline__ unsigned compact_block_total(unsigned wave_total) {
    __shared__ unsigned wave_cnt[4];
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    return wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// emit pass: output index of the wave's first set position = offsets[block] + the totals of the block's earlier waves (16 B of LDS, one barrier)
__device__ __forceinline__ long long compact_wave_base(unsigned wave_total, const long long* __restrict__ offsets, long block) {
    __shared__ unsigned wave_cnt[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_cnt[wave] = wave_total;
    __syncthreads();
    long long base = offsets[block];
    for (int i = 0; i < wave; ++i) base += wave_cnt[i];
    return base;
}

// the whole count pass of a block: partials[slot] = the set positions of the tile that starts at lane position seg (compact_seg, less the
// caller's shift if its grid holds several ranges).  Block-uniform call sites only: there is a barrier inside.
template <int TILE, typename Pos, typename Set>
__device__ __forceinline__ void compact_count(Pos seg, Set set, unsigned* __restrict__ partials, long slot) {
    unsigned long long bal[TILE / 256];
    const unsigned tot = compact_block_total(compact_ballots(seg, set, bal));
    if (threadIdx.x == 0) partials[slot] = tot;
}

// the whole emit pass of a block: body(position, output index) for every set position of the tile, by the lane that owns it.  Output indices
// ascend with the position - rows in order, lanes in order inside a row - from offsets[block].  The index is not bounded here: a body tests
// it against what its caller allocated before it stores anything at it.
template <int TILE, typename Pos, typename Set, typename Body>
__device__ __forceinline__ void compact_emit(Pos seg, Set set, const long long* __restrict__ offsets, long block, Body body) {
    const int lane = threadIdx.x & 63;
    unsigned long long bal[TILE / 256];
    const unsigned tot = compact_ballots(seg, set, bal);
    long long base = compact_wave_base(tot, offsets, block);
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
        const long long idx = base + compact_rank(bal[j]);
        base += __popcll(bal[j]);
        if ((bal[j] >> lane) & 1ull) body(seg + 64 * j, idx);
    }
}

// scan pass, one block of 1024 threads (128 B of LDS): offsets[i] = sum of partials[0 .. i), offsets[n] = the total, which every thread gets
// back.  The partials are walked in chunks of 1024: thread t takes element chunk + t (coalesced loads and stores), the chunk is scanned with
// shuffles inside a wave and the 16 wave totals through LDS, and the running total is carried to the next chunk.  A 49-view scan at
// 1600x1184 has 45 325 partials: 45 chunks.  A caller that reads offsets[] back puts a barrier first.
__device__ __forceinline__ long long compact_scan(const unsigned* __restrict__ partials, long n, long long* __restrict__ offsets) {
    __shared__ long long wave_tot[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long carry = 0;
    for (long c0 = 0; c0 < n; c0 += 1024) {
        const long i = c0 + t;
        const long long s = i < n ? (long long)partials[i] : 0;
        long long inc = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long v = __shfl_up(inc, d);
            if (lane >= d) inc += v;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        long long below = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const long long v = wave_tot[k];
            below += k < wave ? v : 0;
            all += v;
        }
        if (i < n) offsets[i] = carry + below + inc - s;
        carry += all;
        __syncthreads();                             // (wave_tot is rewritten by the next chunk)
    }
    if (t == 0) offsets[n] = carry;
    return carry;
}
