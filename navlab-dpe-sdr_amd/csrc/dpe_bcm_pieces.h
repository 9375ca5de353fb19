// dpe_bcm_pieces.h -- the device pieces the six manifold scans share ("The scan's shared pieces"), included by
// dpe_bcm.hip ahead of scan_body.  Plain forced-inline functions: each scan body is still one straight text that calls them.
// Where a body calls a piece, what the suites promise about it ("a joint row of one receiver equals the plain row", "level l
// equals an axes handle", ...) rests on one copy of that arithmetic.  Not every body calls every piece: where the call moved
// a kernel's registers or hot loops the body keeps that piece's text -- joint_body the recount, subsets_body the pair's index
// and term, axes_body the term, epochs_body its whole tile body (so "a group of one window carries the bits of the
// single-window scan" still rests on two texts kept equal by hand) -- and a change to such a piece is made there as well.
#pragma once

namespace dpe {

constexpr int kPairs = kPtsPerThread / 2;   // a thread's points of a tile, held as pairs (scan_grid_slot)

// The small callables handed to a piece (scan_recount's hit) carry this, so that they are inlined
// with the piece, ahead of the optimiser, and the body is compiled as if the piece's text stood in it
#define DPE_INLINE_LAMBDA __attribute__((always_inline))

// ---- grid points -------------------------------------------------------------------------------------------------------------
// One tile's loads as buffer loads: the descriptor of the tile is built by scalar instructions, the lane's byte offset is
// loop-invariant and the slot offset an immediate, so fetching a tile issues no vector instruction besides the loads.
__device__ __forceinline__ void scan_load_tile(f4 (&g)[2 * kPairs], const f4 *__restrict__ grid, unsigned tile, int tid)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<f4 *>(grid + (size_t)tile * kPtsPerBlock), 0, kPtsPerBlock * (int)sizeof(f4), 0x00020000);
#pragma unroll
    for (int j = 0; j < 2 * kPairs; ++j)
        g[j] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, tid * (int)sizeof(f4), j * 256 * (int)sizeof(f4), 0));
}

// A thread's points of one tile as the packed fp32 math takes them: x, y, z, t of pair p and q = x^2 + y^2 + z^2
struct ScanPts {
    f2 dx[kPairs], dy[kPairs], dz[kPairs], dw[kPairs], q[kPairs];
};

__device__ __forceinline__ void scan_unpack(ScanPts &pt, const f4 (&g)[2 * kPairs])
{
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
        pt.dx[p] = g[2 * p].xy; pt.dy[p] = g[2 * p].zw; pt.dz[p] = g[2 * p + 1].xy; pt.dw[p] = g[2 * p + 1].zw;
        pt.q[p] = pt.dx[p] * pt.dx[p] + pt.dy[p] * pt.dy[p] + pt.dz[p] * pt.dz[p];
    }
}

// The persistent tile walk of one block: tiles tile, tile + stride, ...  Full tiles are unrolled by two so that the prefetch
// alternates between the register sets (no moves carry a tile from one set to the other); the ragged tile, if this block owns
// it, comes last (it is the grid's last tile).  bufA already holds the first tile.  load(regs, tile); tile_body(regs, tile, tag)
// with std::true_type for the ragged tile.  `tile` is the caller's variable: with the counter a local of this function the
// compiler turns the last running-maximum update of the unrolled loop into a branch (one more vector instruction per two tiles).
template <class Load, class TileBody>
__device__ __forceinline__ void scan_walk_tiles(unsigned &tile, unsigned stride, unsigned nFull, unsigned nTiles, f4 (&bufA)[2 * kPairs],
                                                f4 (&bufB)[2 * kPairs], const Load &load, const TileBody &tile_body)
{
    for (;;) {
        if (tile >= nFull) break;
        const unsigned t1 = tile + stride;
        if (t1 < nTiles) load(bufB, t1);
        tile_body(bufA, tile, std::false_type{});
        tile = t1;
        if (tile >= nFull) {
#pragma unroll
            for (int j = 0; j < 2 * kPairs; ++j) bufA[j] = bufB[j];   // (once per walk, for the ragged tile below)
            break;
        }
        const unsigned t2 = tile + stride;
        if (t2 < nTiles) load(bufA, t2);
        tile_body(bufB, tile, std::false_type{});
        tile = t2;
    }
    if (tile < nTiles) tile_body(bufA, tile, std::true_type{});
}

// ---- score banks in LDS ------------------------------------------------------------------------------------------------------
// |c0 + w (c1 - c0)|^2 = A + w (B + w C): the interpolated magnitude needs two FMAs per pair.  Entry i = (row, j) of a bank of
// rows of nEnt as {A, B, 0, C}: one address register serves the ds_read_b64 {A, B} and the ds_read_b32 {C} (immediate offset
// 12; the gap keeps the compiler from fusing them into a slower ds_read_b96).  Entry nEnt - 1 of a row can never be a valid
// lower neighbour: it is the all-zero slot that out-of-window indices are clamped to (contribution exactly 0).
// Fills n = rows * nEnt entries of one bank into dst.  A wave's 64 points land on a few neighbouring entries (the index moves
// by << 1 entry per grid step), so the 16-byte stride is conflict-free as long as a wave spans < 16 entries.
template <bool COMPACT = false>
__device__ __forceinline__ void scan_fill_bank(float4 *dst, const float2 *__restrict__ bw, int n, int nEnt, int tid)
{
    float *dstF = reinterpret_cast<float *>(dst);   // COMPACT (scan_body only): 12-byte entries {A, B, C}
    for (int i = tid; i < n; i += 256) {
        const int k = i / nEnt, j = i - k * nEnt;
        if (j + 1 < nEnt) {
            const float2 c0 = bw[(size_t)k * nEnt + j], c1 = bw[(size_t)k * nEnt + j + 1];
            const float dr = c1.x - c0.x, di = c1.y - c0.y;
            const float eA = c0.x * c0.x + c0.y * c0.y, eB = 2.f * (c0.x * dr + c0.y * di), eC = dr * dr + di * di;
            if (COMPACT) { dstF[3 * i] = eA; dstF[3 * i + 1] = eB; dstF[3 * i + 2] = eC; }
            else dst[i] = make_float4(eA, eB, 0.f, eC);
        } else {
            if (COMPACT) { dstF[3 * i] = 0.f; dstF[3 * i + 1] = 0.f; dstF[3 * i + 2] = 0.f; }
            else dst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

// ---- index and term ----------------------------------------------------------------------------------------------------------
// The fractional bank index of the two points of pair p against SV s (dpe_bcm.hip's head: SECOND = the position manifold's
// second-order range expansion, else the velocity manifold's linear form)
template <bool SECOND>
__device__ __forceinline__ f2 scan_pair_index(const ScanPts &pt, int p, const BcmSvDev &s)
{
    if (SECOND) {
        f2 a = pt.dx[p] * s.ue;
        a = __builtin_elementwise_fma(pt.dy[p], f2{s.un, s.un}, a);
        a = __builtin_elementwise_fma(pt.dz[p], f2{s.uu, s.uu}, a);
        f2 x = pt.dw[p] - a;
        const f2 t = __builtin_elementwise_fma(-a, a, pt.q[p]);          // q - a^2
        x = __builtin_elementwise_fma(t, f2{s.h, s.h}, x);               // + (q - a^2) / (2 range)
        return __builtin_elementwise_fma(x, f2{s.g, s.g}, f2{s.idx0, s.idx0});
    }
    f2 idx = __builtin_elementwise_fma(pt.dw[p], f2{s.g, s.g}, f2{s.idx0, s.idx0});
    idx = __builtin_elementwise_fma(pt.dx[p], f2{-s.h, -s.h}, idx);
    idx = __builtin_elementwise_fma(pt.dy[p], f2{-s.pad0, -s.pad0}, idx);
    return __builtin_elementwise_fma(pt.dz[p], f2{-s.pad1, -s.pad1}, idx);
}

// The same index for ONE point (it) in scalar fp32 -- the fast path's own expression, operation for operation
template <bool SECOND>
__device__ __forceinline__ float scan_point_index(const ScanPts &pt, int it, const BcmSvDev &s)
{
    const float px = pt.dx[it >> 1][it & 1], py = pt.dy[it >> 1][it & 1], pz = pt.dz[it >> 1][it & 1];
    const float pw = pt.dw[it >> 1][it & 1], pq = pt.q[it >> 1][it & 1];
    if (SECOND) {
        const float a = fmaf(pz, s.uu, fmaf(py, s.un, px * s.ue));
        float x = pw - a;
        x = fmaf(fmaf(-a, a, pq), s.h, x);
        return fmaf(x, s.g, s.idx0);
    }
    return fmaf(pz, -s.pad1, fmaf(py, -s.pad0, fmaf(px, -s.h, fmaf(pw, s.g, s.idx0))));
}

// Tensor-product grids (axes_body, refine_body): the part of the index that the row (x, y, z; q = x^2 + y^2 + z^2) fixes; the
// point's index is fma(t, s.g, B)
template <bool SECOND>
__device__ __forceinline__ float axes_row_index(float x, float y, float z, float q, const BcmSvDev &s)
{
    if (SECOND) {
        const float a = fmaf(z, s.uu, fmaf(y, s.un, x * s.ue));
        return fmaf(fmaf(fmaf(-a, a, q), s.h, -a), s.g, s.idx0);
    }
    return fmaf(z, -s.pad1, fmaf(y, -s.pad0, fmaf(x, -s.h, s.idx0)));
}

__device__ __forceinline__ unsigned floor_entry(float id)
{
    int ei;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ei) : "v"(id));          // (int)floor(id), saturating
    return (unsigned)ei;
}

// One (point, SV) term from the fractional index id and the SV's bank row bk: the reference's floor / floor(+1) linear
// interpolation and |.|^L.  CLAMP: an index outside the bank (negative -> huge) goes to the zero slot `last`, and emax keeps
// the largest entry seen.  COMPACT (scan_body only): bk is the whole bank of 12-byte entries {A, B, C} and the SV's row starts
// `row` entries into it (the row is added to the entry before the scaling by 12, not to the pointer: one address register less).
template <int LP, bool CLAMP, bool COMPACT = false>
__device__ __forceinline__ float scan_term(float id, const void *bk, unsigned last, unsigned &emax, int lpower, size_t row = 0)
{
    const float wgt = __builtin_amdgcn_fractf(id);                 // id - floor(id)
    unsigned e = floor_entry(id);
    if (CLAMP) {
        e = min(e, last);
        emax = max(emax, e);
    }
    float m2;
    if (COMPACT) {
        const float *bf = static_cast<const float *>(bk) + (row + e) * 3;
        m2 = fmaf(wgt, fmaf(wgt, bf[2], bf[1]), bf[0]);
    } else {
        const float4 *b4 = static_cast<const float4 *>(bk);
        const float2 ab = *reinterpret_cast<const float2 *>(&b4[e]);
        m2 = fmaf(wgt, fmaf(wgt, b4[e].w, ab.y), ab.x);
    }
    if (LP == 1) return __builtin_amdgcn_sqrtf(__builtin_fabsf(m2));    // raw v_sqrt_f32 (1 ulp)
    if (LP == 2) return m2;
    return powf(__builtin_amdgcn_sqrtf(__builtin_fabsf(m2)), (float)lpower);
}

// Both points of pair p against SV s
template <int LP, bool SECOND, bool CLAMP, bool COMPACT = false>
__device__ __forceinline__ f2 scan_pair_term(const ScanPts &pt, int p, const BcmSvDev &s, const void *bk, unsigned last, unsigned &emax, int lpower,
                                             size_t row = 0)
{
    const f2 idx = scan_pair_index<SECOND>(pt, p, s);
    const float c0 = scan_term<LP, CLAMP, COMPACT>(idx[0], bk, last, emax, lpower, row);
    const float c1 = scan_term<LP, CLAMP, COMPACT>(idx[1], bk, last, emax, lpower, row);
    return f2{c0, c1};
}

// Whether the index id falls on the zero slot (outside the bank)
__device__ __forceinline__ bool scan_oob(float id, unsigned last) { return min(floor_entry(id), last) == last; }

// Out-of-window bookkeeping off the fast path: the tile's (point, SV) pairs recounted one by one, for a thread that hit the zero
// slot.  hit(k, n) is called for every pair of SV k, with n = 1 where the pair is out of the window and 0 where it is not (a
// count, not a branch: the bodies that count in a register add it); the ragged tile's padded points (base + it * 256 >= G)
// are skipped.
template <bool SECOND, bool RAGGED, class Hit>
__device__ __forceinline__ void scan_recount(const ScanPts &pt, const BcmSvDev *svw, int K, unsigned last, long long base, long long G, const Hit &hit)
{
    for (int it = 0; it < kPtsPerThread; ++it) {
        if (RAGGED && base + it * 256 >= G) continue;
        for (int k = 0; k < K; ++k) hit(k, scan_oob(scan_point_index<SECOND>(pt, it, svw[k]), last) ? 1u : 0u);
    }
}

// ---- rows and keys -----------------------------------------------------------------------------------------------------------
// A tile's scores into its row (srow: the tile's first float, wave-uniform).  Written once and never read back: non-temporal
// stores keep ~0.8 GB per 256-window call from lingering as dirty L2 / Infinity-Cache lines whose write-back would run into the
// NEXT call's first kernels (measured: the following DC-sum kernel 25 -> 13 us, step 0.863 -> 0.851 ms)
template <bool RAGGED>
__device__ __forceinline__ void scan_store_row(float *srow, const f2 (&score)[kPairs], long long base, long long G, int tid)
{
#pragma unroll
    for (int it = 0; it < kPtsPerThread; ++it) {
        if (RAGGED && base + it * 256 >= G) continue;
        __builtin_nontemporal_store(score[it >> 1][it & 1], &srow[it * 256 + tid]);
    }
}

// Per-lane running maximum: a lane visits its points in increasing index order, so a strict "greater" keeps the first maximum.
// The maximum remembers (tile, it) of its point; the index is formed once, after the tile walk.
template <bool RAGGED>
__device__ __forceinline__ void scan_track_max(const f2 (&score)[kPairs], long long base, long long G, unsigned tile, float &bestSc,
                                               unsigned int &bestTile, unsigned int &bestIt)
{
#pragma unroll
    for (int it = 0; it < kPtsPerThread; ++it) {
        const float sc = score[it >> 1][it & 1];
        if ((!RAGGED || base + it * 256 < G) && sc > bestSc) { bestSc = sc; bestTile = tile; bestIt = (unsigned)it; }
    }
}

// The same for one of several maxima a body keeps beside the main one (per receiver, per subset): the point is remembered in
// ONE register, as tile * kPtsPerThread + it
template <bool RAGGED>
__device__ __forceinline__ void scan_track_max(const f2 (&score)[kPairs], long long base, long long G, unsigned tile, float &bestSc, unsigned int &bestAt)
{
#pragma unroll
    for (int it = 0; it < kPtsPerThread; ++it) {
        const float sc = score[it >> 1][it & 1];
        if ((!RAGGED || base + it * 256 < G) && sc > bestSc) { bestSc = sc; bestAt = tile * (unsigned)kPtsPerThread + (unsigned)it; }
    }
}

// local index (within this rank's shard) of the point scan_track_max remembered, for the lane tid
__device__ __forceinline__ unsigned int scan_local_index(unsigned int tile, unsigned int it, int tid)
{
    return tile * (unsigned int)kPtsPerBlock + it * 256u + (unsigned int)tid;
}

// (score, index) as one 64-bit key: larger score wins, ties -> smaller index (thrust::max_element, :2589); score < 0: no point
__device__ __forceinline__ unsigned long long pack_key(float score, unsigned int index)
{
    return score < 0.f ? 0ull : (((unsigned long long)__float_as_uint(score) << 32) | (unsigned long long)(0xFFFFFFFFu - index));
}

__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long best)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    return best;
}

__device__ __forceinline__ unsigned int wave_sum(unsigned int n)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    return n;
}

// the four waves' keys, left in LDS by their first lanes (stride: elements between consecutive waves' slots)
__device__ __forceinline__ unsigned long long block_max_key(const unsigned long long *sKey, int stride = 1)
{
    unsigned long long b = sKey[0];
    b = sKey[stride] > b ? sKey[stride] : b;
    b = sKey[2 * stride] > b ? sKey[2 * stride] : b;
    b = sKey[3 * stride] > b ? sKey[3 * stride] : b;
    return b;
}

// Thread 0's last step in every scan: the block's key and out-of-window count into the window's slot.  Integer max: order-
// independent.  RETURNING atomics: their results are waited for before this block takes its ticket (scan_publish), which orders
// them without a release fence -- on gfx950 an agent-scope fence writes back the XCD's whole L2 (all the dirty score lines)
__device__ __forceinline__ void scan_post_key(unsigned long long *key, unsigned long long *oob, unsigned long long b, unsigned int n)
{
    unsigned long long seen = atomicMax(key, b);
    if (n) seen += atomicAdd(oob, (unsigned long long)n);
    asm volatile("" ::"v"(seen) : "memory");   // keep the returns (and the s_waitcnt they imply) alive, and the ticket below them
}

}  // namespace dpe
