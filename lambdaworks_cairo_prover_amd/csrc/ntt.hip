// Stark252 NTT passes for gfx950. See ntt.h for the structure and DESIGN.md section 4.1 for the twiddle bookkeeping.
#include "ntt.h"
#include <algorithm>

// Compile-time variants (A/B: tools/sweep_ntt_variants.sh).
// 1: the strided passes of whole transforms read every stage's twiddles from that stage's own dense table (NttEngine::stage_tables);
// 0: from the single table w_M^e with a stride, as the LDE passes do.  Same values either way.
#ifndef SP_NTT_STAGE_TW
#define SP_NTT_STAGE_TW 1
#endif
// A fresh work-group competes with up to three computing ones for issue slots and, as the youngest, loses: raise its
// priority until its tile and twiddle loads are on their way (SP_NTT_PRIO & 1: 34 x 2^22 10.95 -> 10.7 ms); doing the same
// for the final stores (& 2) changes nothing (profiles/r02_ntt_prio_sweep.txt)
#ifndef SP_NTT_PRIO
#define SP_NTT_PRIO 1
#endif
// a pass with an odd number of stages runs one of them as a single radix-2 stage - a whole LDS round trip for one stage
// instead of two: geometry() trades stages between two odd passes where the tile allows it (14 = 8 + 6 instead of 7 + 7)
#ifndef SP_NTT_EVEN_SPLIT
#define SP_NTT_EVEN_SPLIT 1
#endif

namespace sp {

// ---------------------------------------------------------------------------------------------- device helpers
__device__ __forceinline__ fe ld_fe(const fe* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 lo = q[0], hi = q[1];
    fe r;
    r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = lo.z; r.v[3] = lo.w;
    r.v[4] = hi.x; r.v[5] = hi.y; r.v[6] = hi.z; r.v[7] = hi.w;
    return r;
}
__device__ __forceinline__ void st_fe(fe* p, const fe& a) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
    q[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}
// LDS array of field elements (the tile, the twiddle table): two planes of 16-byte halves so that consecutive lanes touch
// consecutive 16-byte slots.
struct LdsPlanes {
    uint4 *lo, *hi;
    __device__ __forceinline__ fe ld(uint32_t i) const {
        uint4 a = lo[i], b = hi[i];
        fe r;
        r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
        r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
        return r;
    }
    __device__ __forceinline__ void st(uint32_t i, const fe& a) const {
        lo[i] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
        hi[i] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
    }
};
__device__ __forceinline__ uint32_t bitrev(uint32_t x, uint32_t bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }

// The template flags of one ntt_pass_kernel instantiation as a type, so that every piece below keeps only its own address math.
template <bool DIF_, int LOADM_, int STOREM_, bool CONTIG_, bool GTW_>
struct PassFlags {
    static constexpr bool DIF = DIF_, CONTIG = CONTIG_, GTW = GTW_;
    static constexpr int LOADM = LOADM_, STOREM = STOREM_;
};
constexpr int BPT = (1 << (NTT_TILE_LOG - 1)) / NTT_THREADS;   // butterflies per thread and stage (at most)

// ---------------------------------------------------------------------------------------------- tile map
// Which tile of which vector a work-group runs, and where the tile's elements live: a tile is R = 2^r rows at stride 2^s with
// G = 2^g adjacent elements per row (one row of 2^r contiguous elements times G rows-to-be for the s = 0 pass).
template <class P>
struct TileMap {
    uint32_t r, g, s;          // s: local (address) stride; the twiddles use the global stride s + a.tw_shift
    uint32_t logL;             // size of the array this pass addresses
    uint32_t tile, lo0, hi;    // strided tiles: tile = (hi, lo0 >> g)
    uint32_t tw_low;           // low bits of the twiddle exponent: a.tw_low, plus the local coset in the coset-major LDE
    const fe* src;
    fe* dst;

    __device__ __forceinline__ explicit TileMap(const NttPassArgs& a) : r(a.r), g(a.g), s(a.s), logL(a.logL), lo0(0), hi(0), tw_low(a.tw_low) {
        // vector index fastest: consecutive work-groups run the same tile of different vectors, so the twiddles they gather
        // (the same table entries for every vector) are L2 hits for all but the first of them.
        // Work-groups are dealt round-robin to the 8 XCDs (each with its own L2): pin tile t to XCD t mod 8 and let that XCD
        // run the tile for all vectors back to back  (id = slot * 8 + t % 8, slot = (t / 8) * batch + vec).
        uint32_t vec;
        if (a.xcd_map) {
            const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
            const uint32_t tg = slot / a.batch;
            vec = slot - tg * a.batch;
            tile = (tg << 3) | xcd;
        } else {
            tile = blockIdx.x / a.batch;
            vec = blockIdx.x - tile * a.batch;
        }
        // coset-major LDE: "vector" = (column v, local coset cl); every coset is its own array of 2^logL evaluations
        if (a.coset_count) {
            const uint32_t v = vec / a.coset_count, cl = vec - v * a.coset_count;
            src = a.src + (uint64_t)v * a.src_vec_stride + (uint64_t)cl * a.src_coset_stride;
            dst = a.dst + (uint64_t)v * a.dst_vec_stride + (uint64_t)cl * a.dst_coset_stride;
            tw_low |= cl << a.shard_log;
        } else {
            src = a.src + (uint64_t)vec * a.src_vec_stride;
            dst = a.dst + (uint64_t)vec * a.dst_vec_stride;
        }
        if (!P::CONTIG) {
            uint32_t lo_tiles = 1u << (s - g);
            lo0 = (tile & (lo_tiles - 1)) << g;
            hi = tile >> (s - g);
        }
    }
    __device__ __forceinline__ uint32_t R() const { return 1u << r; }
    __device__ __forceinline__ uint32_t G() const { return 1u << g; }
    __device__ __forceinline__ uint32_t TILE() const { return R() << g; }
    // position (in the 2^logL working array) of tile element (t, gl)
    __device__ __forceinline__ uint32_t position(uint32_t t, uint32_t gl) const {
        if (P::CONTIG) {
            if (P::LOADM == NTT_LOAD_GATHER_BITREV || P::STOREM == NTT_STORE_SCATTER_BITREV)
                return (bitrev((tile << g) + gl, logL - r) << r) + t;   // row whose bit-reversed index is adjacent
            return (tile << (r + g)) + (gl << r) + t;
        }
        return (hi << (s + r)) + (t << s) + lo0 + gl;
    }
    // index of (t, gl) in the LDS tile
    __device__ __forceinline__ uint32_t lidx(uint32_t t, uint32_t gl) const { return P::CONTIG ? (gl << r) + t : (t << g) + gl; }
    // natural-order index of (t, gl) on the far side of a bit-reversal gather or scatter: x[rev(pos)]
    __device__ __forceinline__ uint32_t bitrev_index(uint32_t t, uint32_t gl) const { return (bitrev(t, r) << (logL - r)) + (tile << g) + gl; }
};

// ---------------------------------------------------------------------------------------------- twiddles
// Stage J = a.s + j of a pass pairs positions P and P + 2^(J-1) with w = w_(2^J)^(P mod 2^(J-1)).  The s = 0 pass uses the
// pass-local table w_R^(+-e) (R/2 entries in LDS).  A strided pass stages the twiddles
// of its own butterflies: w_M^(((i << a.s) + column) << (logM - a.s - j)), i = row mod 2^(j-1); the global column of
// local column c is (c << shard_log) | shard_rank.  Stages j < r go to LDS (entry (2^(j-1) - 1 + i) * G + gl), the
// twiddles of stage r serve one butterfly each and go straight to registers.  There is no inter-pass twiddle product.
// With a.stage_tw the same value w_(2^J)^x, J = a.s + j, x = (i << a.s) + column, comes from stage J's own dense table
// (entry 2^(J-1) + x of the pyramid): the G columns of a tile row are G adjacent entries, so no fetched 128-byte line
// carries twiddles of other stages (every 2^(logM-J)-th entry of the single table: a line per twiddle from stride 4 on).
// Twiddles are always canonical, so every product is fe_mul_lazy(data, twiddle).
constexpr int twiddle_regs(bool gtw, bool contig) { return (gtw && !contig) ? BPT : 1; }   // stage-r twiddles a thread keeps in registers

// w_(2^J)^x (DIF: its inverse) for stage j = jm1 + 1 of this pass, row index i, local column gl, from the transform's table
template <class P>
__device__ __forceinline__ fe global_tw(const NttPassArgs& a, const TileMap<P>& m, uint32_t jm1, uint32_t i, uint32_t gl) {
    const uint32_t sg = m.s + a.tw_shift;    // global stride of this pass
    const uint32_t col = ((m.lo0 + gl) << a.tw_shift) | m.tw_low;
    const uint32_t x = (i << sg) + col, h = 1u << (sg + jm1);   // w_(2^J)^x, x < h = 2^(J-1)
    // single table: entry x << (logM - J); pyramid: entry h + x.  The inverse butterfly mirrors x -> h - x in both:
    // w^-1 = -w_(2^J)^(2^(J-1) - e), so it computes (y - x) times a forward-table entry (and times -1 for e = 0) and one table
    // serves both directions.
    const bool pyr = SP_NTT_STAGE_TW && a.stage_tw;
    const uint32_t sh = pyr ? 0u : a.logM - sg - jm1 - 1u, off = pyr ? h : 0u;
    if (!P::DIF) return ld_fe(a.big_tw + off + (x << sh));
    if (x == 0) return fe_neg_one();
    return ld_fe(a.big_tw + off + ((h - x) << sh));
}

// ---------------------------------------------------------------------------------------------- the phases of a pass
template <class P>
__device__ __forceinline__ void load_tile(const TileMap<P>& m, uint32_t tid, const LdsPlanes& L) {
    constexpr int LU = 4;   // loads in flight per thread
    const uint32_t r = m.r, g = m.g, R = m.R(), G = m.G(), TILE = m.TILE();
    for (uint32_t e0 = tid; e0 < TILE; e0 += NTT_THREADS * LU) {
        fe xs[LU];
        uint32_t li[LU];
#pragma unroll
        for (int q = 0; q < LU; ++q) {
            const uint32_t e = e0 + q * NTT_THREADS;
            if (e >= TILE) continue;
            uint32_t t, gl;
            if (P::CONTIG && P::LOADM == NTT_LOAD_INPLACE) {
                t = e & (R - 1); gl = e >> r;
                xs[q] = ld_fe(m.src + m.position(t, gl));
            } else if (P::CONTIG) {  // gather from the natural-order source
                gl = e & (G - 1); t = e >> g;
                xs[q] = ld_fe(m.src + m.bitrev_index(t, gl));
            } else {
                gl = e & (G - 1); t = e >> g;
                uint32_t pos = m.position(t, gl);
                if (P::LOADM == NTT_LOAD_EXPAND) xs[q] = ld_fe(m.src + (pos >> m.s));  // s = local log2(cosets held)
                else xs[q] = ld_fe(m.src + pos);
            }
            li[q] = m.lidx(t, gl);
        }
#pragma unroll
        for (int q = 0; q < LU; ++q)
            if (e0 + q * NTT_THREADS < TILE) L.st(li[q], xs[q]);
    }
}

__device__ __forceinline__ fe store_form(const NttPassArgs& a, const fe& x) { return a.weak_out ? fe_reduce_lazy_2p(x) : fe_canonical_lazy(x); }
template <class P>
__device__ __forceinline__ void store_tile(const NttPassArgs& a, const TileMap<P>& m, uint32_t tid, const LdsPlanes& L) {
    if (SP_NTT_PRIO & 2) __builtin_amdgcn_s_setprio(3);
    const uint32_t r = m.r, g = m.g, R = m.R(), G = m.G(), TILE = m.TILE();
    fe scal;
    const bool has_scalar = a.scalar != nullptr;
    if (has_scalar) scal = ld_fe(a.scalar);
    for (uint32_t e = tid; e < TILE; e += NTT_THREADS) {
        uint32_t t, gl;
        if (P::CONTIG && P::STOREM == NTT_STORE_INPLACE) { t = e & (R - 1); gl = e >> r; }
        else { gl = e & (G - 1); t = e >> g; }
        fe x = L.ld(m.lidx(t, gl));
        uint32_t pos = m.position(t, gl);
        uint32_t didx = pos;
        if (P::CONTIG && P::STOREM == NTT_STORE_SCATTER_BITREV) didx = m.bitrev_index(t, gl);
        if (P::DIF && a.post_table) x = fe_mul_lazy(x, ld_fe(a.post_table + didx));
        if (has_scalar) x = fe_mul_lazy(x, scal);
        st_fe(m.dst + didx, store_form(a, x));
    }
}

// One pass = r consecutive radix-2 stages of the plain in-place transform of size 2^logM on a tile of R = 2^r rows at
// stride 2^s (G adjacent elements per row).  Template flags are compile-time so each instantiation keeps only its own
// address math.
//  * DIT (Cooley-Tukey, bit-reversed in -> natural out): stage J = a.s + j pairs positions P and P + 2^(J-1) and computes
//    (u, v) -> (u + v w, u - v w) with w = w_(2^J)^(P mod 2^(J-1)).
//  * DIF (Gentleman-Sande, natural in -> bit-reversed out, inverse roots, unscaled): the same pairs in the opposite stage
//    order, (x, y) -> (x + y, (x - y) w^-1); with the transform's table (GTW) the butterfly computes (y - x) times what
//    global_tw returns.
//  * Deferred reduction (fp.h): p > 2^251, so every 256-bit value is < 32p.  Pass input < 2p.  DIT: t = v w < 2p and the
//    outputs u + t, u - t + 2p grow by 2p per stage - no correction for the <= 10 stages of a pass.  DIF: x + y doubles
//    the bound, (y - x + kb p) w is < 2p again; the sum is brought back below 2p every third stage (kb = 2, 4, 8).
//    Stores: fe_reduce_lazy_2p on every pass but the last of a transform (a.weak_out), fe_canonical_lazy on the last.
// The phases: tile map (TileMap), twiddles, load_tile | the stages | store_tile.  The twiddle staging, the radix-4 units of both
// directions, the radix-2 stage and the DIT pass's fused last-pair store stand in the body: as functions they compile to other
// code in some instantiation - registers, compare/select or carry instructions (profiles/ntt_pass_phases.txt).
template <bool DIF, int LOADM, int STOREM, bool CONTIG, bool GTW>
__global__ void __launch_bounds__(NTT_THREADS) ntt_pass_kernel(NttPassArgs a) {
    using P = PassFlags<DIF, LOADM, STOREM, CONTIG, GTW>;
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    if (SP_NTT_PRIO & 1) __builtin_amdgcn_s_setprio(3);
    const uint32_t r = a.r, g = a.g;
    const uint32_t R = 1u << r, G = 1u << g, TILE = R << g;
    const LdsPlanes L{smem, smem + TILE};
    const LdsPlanes Tw{smem + 2 * TILE, smem + 2 * TILE + (GTW ? (CONTIG ? R : (a.radix4 ? (TILE >> 2) : (TILE >> 1))) : (R >> 1))};
    const uint32_t tid = threadIdx.x;
    const TileMap<P> m(a);
    // ------------------------------------------------------------------ twiddles (global table: contiguous tile, strided tile; pass-local table)
    fe tw_last[twiddle_regs(GTW, CONTIG)];
    fe tw_pen;   // strided passes in pairs: the stage-(r-1) twiddle of this thread's last unit
    if (GTW && CONTIG) {
        // contiguous tile: the twiddle depends on the row only, entry 2^(j-1) - 1 + i for stage j (R - 1 entries)
        for (uint32_t x = tid; x + 1 < R; x += NTT_THREADS) {
            const uint32_t y = x + 1u, jm1 = 31u - __clz(y);
            Tw.st(x, global_tw(a, m, jm1, y - (1u << jm1), 0u));
        }
    } else if (GTW) {
        if (r >= 1) {
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                // stage-r butterflies of this thread: tid + q * threads, or - two stages per round trip (a.radix4) - the two
                // of its radix-4 unit, tid and tid + TILE/4
                const uint32_t b = tid + q * (a.radix4 ? (TILE >> 2) : (uint32_t)NTT_THREADS);
                if (b < (TILE >> 1)) tw_last[q] = global_tw(a, m, r - 1, b >> g, b & (G - 1));
            }
            // in pairs the twiddle of stage r - 1 also serves one unit only (row i = unit index): a register as well, and the
            // LDS table ends with stage r - 2 (40 KB per work-group instead of 48: four work-groups per CU)
            if (a.radix4 && r >= 2 && tid < (TILE >> 2)) tw_pen = global_tw(a, m, r - 2, tid >> g, tid & (G - 1));
            const uint32_t cnt = (a.radix4 ? (TILE >> 2) : (TILE >> 1)) - G;
            fe tmp[BPT];
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const uint32_t x = tid + q * NTT_THREADS;
                if (x < cnt) {
                    const uint32_t y = (x >> g) + 1u;
                    const uint32_t jm1 = 31u - __clz(y);                 // j - 1
                    tmp[q] = global_tw(a, m, jm1, y - (1u << jm1), x & (G - 1));
                }
            }
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const uint32_t x = tid + q * NTT_THREADS;
                if (x < cnt) Tw.st(x, tmp[q]);
            }
        }
    } else {
        for (uint32_t i = tid; i < (R >> 1); i += NTT_THREADS) Tw.st(i, ld_fe(a.small_tw + i));
    }
    // ------------------------------------------------------------------ load
    load_tile(m, tid, L);
    if (SP_NTT_PRIO & 1) __builtin_amdgcn_s_setprio(0);
    __syncthreads();

    // ------------------------------------------------------------------ radix-2 stages
    const uint32_t NB = TILE >> 1;
    uint32_t kb = 2;   // DIF: every element is < kb * p
    // DIT passes: after an odd leading stage, two stages per LDS round trip - a radix-4 unit of the four rows
    // t0 + {0, 1, 2, 3} * 2^(j-1) stays in registers between stage j and stage j + 1 (one unit per thread, TILE/4 units)
    const bool r4 = a.radix4 != 0;
    // DIF runs the stages downwards: pairs (r, r-1), (r-2, r-3), ... first, an odd stage 1 last
    if (DIF && r4) {
        for (uint32_t jt = r; jt >= 2; jt -= 2) {
            const uint32_t j = jt - 1, half = 1u << (j - 1);       // stages j + 1 (first) and j
            const uint32_t u = tid;
            const bool foldA = kb == 8;
            const uint32_t kbB = foldA ? 2u : 2u * kb;             // bound of the stage-(j+1) outputs
            const bool foldB = kbB == 8;
            if (u < (TILE >> 2)) {
                uint32_t gl, bq;
                if (CONTIG) { bq = u & ((R >> 2) - 1); gl = u >> (r - 2); } else { gl = u & (G - 1); bq = u >> g; }
                const uint32_t i = bq & (half - 1);
                const uint32_t t0 = ((bq >> (j - 1)) << (j + 1)) | i;
                const uint32_t l0 = m.lidx(t0, gl), l1 = m.lidx(t0 + half, gl), l2 = m.lidx(t0 + 2 * half, gl), l3 = m.lidx(t0 + 3 * half, gl);
                fe wa, wb, wc;          // stage j + 1: wb (rows 0, 2), wc (rows 1, 3); stage j: wa
                bool has_wa = true;
                if (GTW) {
                    if (j + 1 == r) { wb = tw_last[0]; wc = tw_last[BPT - 1]; wa = tw_pen; }
                    else { wb = Tw.ld(((2 * half - 1u + i) << g) + gl); wc = Tw.ld(((3 * half - 1u + i) << g) + gl);
                           wa = Tw.ld(((half - 1u + i) << g) + gl); }
                } else {                // pass-local table w_R^-e
                    wb = Tw.ld(i << (r - j - 1)); wc = Tw.ld((i + half) << (r - j - 1));
                    if (j > 1) wa = Tw.ld(i << (r - j)); else has_wa = false;
                }
                fe x0 = L.ld(l0), x1 = L.ld(l1), x2 = L.ld(l2), x3 = L.ld(l3);
                // stage j + 1: (x0, x2), (x1, x3)
                fe a0 = fe_add_raw(x0, x2), a1 = fe_add_raw(x1, x3);
                if (foldA) { a0 = fe_reduce_lazy_2p(a0); a1 = fe_reduce_lazy_2p(a1); }
                fe a2 = GTW ? fe_sub_add_kp(x2, x0, kb) : fe_sub_add_kp(x0, x2, kb);
                fe a3 = GTW ? fe_sub_add_kp(x3, x1, kb) : fe_sub_add_kp(x1, x3, kb);
                a2 = fe_mul_lazy(a2, wb); a3 = fe_mul_lazy(a3, wc);
                // stage j: (a0, a1), (a2, a3); every input is < kbB p
                fe s0 = fe_add_raw(a0, a1), s2 = fe_add_raw(a2, a3);
                if (foldB) { s0 = fe_reduce_lazy_2p(s0); s2 = fe_reduce_lazy_2p(s2); }
                fe d1 = GTW ? fe_sub_add_kp(a1, a0, kbB) : fe_sub_add_kp(a0, a1, kbB);
                fe d3 = GTW ? fe_sub_add_kp(a3, a2, kbB) : fe_sub_add_kp(a2, a3, kbB);
                if (has_wa) { d1 = fe_mul_lazy(d1, wa); d3 = fe_mul_lazy(d3, wa); }
                L.st(l0, s0); L.st(l1, d1); L.st(l2, s2); L.st(l3, d3);
            }
            kb = foldB ? 2u : 2u * kbB;
            __syncthreads();
        }
    }
    // radix-2 stages: all of them without a.radix4; with it the odd leading stage of a DIT pass / the odd last stage (1) of DIF
    const uint32_t singles = r4 ? (r & 1u) : r;
    uint32_t jj = 1;
    for (; jj <= singles; ++jj) {
        const uint32_t j = (DIF && !r4) ? r + 1 - jj : jj;     // (DIF with pairs: only stage 1 is left)
        const uint32_t half = 1u << (j - 1);
        const bool fold = DIF && kb == 8;   // the sums of this stage would reach 16p: bring them back below 2p
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            const uint32_t b = tid + q * NTT_THREADS;
            if (b >= NB) continue;
            uint32_t bf, gl;
            if (CONTIG) { bf = b & ((R >> 1) - 1); gl = b >> (r - 1); } else { gl = b & (G - 1); bf = b >> g; }
            const uint32_t i = bf & (half - 1);
            const uint32_t t0 = 2u * bf - i;                    // ((bf >> (j-1)) << j) | i
            const uint32_t i0 = m.lidx(t0, gl), i1 = m.lidx(t0 + half, gl);
            fe w;
            bool has_w = true;
            if (GTW && CONTIG) w = Tw.ld(half - 1u + i);
            else if (GTW) { if (j == r) w = tw_last[q]; else w = Tw.ld(((half - 1u + i) << g) + gl); }
            else if (j > 1) w = Tw.ld(i << (r - j));
            else has_w = false;                                 // w_2^0 = 1
            fe x = L.ld(i0), y = L.ld(i1);
            if (!DIF) {
                if (has_w) y = fe_mul_lazy(y, w);               // stage 1 of the s = 0 pass: y < 2p already
                L.st(i0, fe_add_raw(x, y));
                L.st(i1, fe_sub_add_2p(x, y));
            } else {
                fe sum = fe_add_raw(x, y);
                if (fold) sum = fe_reduce_lazy_2p(sum);
                fe d = GTW ? fe_sub_add_kp(y, x, kb) : fe_sub_add_kp(x, y, kb);
                if (has_w) d = fe_mul_lazy(d, w);
                L.st(i0, sum);
                L.st(i1, d);
            }
        }
        kb = fold ? 2u : 2u * kb;
        __syncthreads();
    }
    if (!DIF) {
        for (; jj + 1 <= r; jj += 2) {
            const uint32_t j = jj, half = 1u << (j - 1);
            const uint32_t u = tid;
            if (u < (TILE >> 2)) {
                uint32_t gl, bq;
                if (CONTIG) { bq = u & ((R >> 2) - 1); gl = u >> (r - 2); } else { gl = u & (G - 1); bq = u >> g; }
                const uint32_t i = bq & (half - 1);
                const uint32_t t0 = ((bq >> (j - 1)) << (j + 1)) | i;
                const uint32_t l0 = m.lidx(t0, gl), l1 = m.lidx(t0 + half, gl), l2 = m.lidx(t0 + 2 * half, gl), l3 = m.lidx(t0 + 3 * half, gl);
                fe wa, wb, wc;
                bool has_wa = true;
                if (GTW && CONTIG) {
                    wa = Tw.ld(half - 1u + i); wb = Tw.ld(2 * half - 1u + i); wc = Tw.ld(3 * half - 1u + i);
                } else if (GTW) {
                    if (j + 1 == r) { wa = tw_pen; wb = tw_last[0]; wc = tw_last[BPT - 1]; }
                    else { wa = Tw.ld(((half - 1u + i) << g) + gl);
                           wb = Tw.ld(((2 * half - 1u + i) << g) + gl); wc = Tw.ld(((3 * half - 1u + i) << g) + gl); }
                } else {   // pass-local table w_R^e
                    if (j > 1) wa = Tw.ld(i << (r - j)); else has_wa = false;   // stage 1: w = 1, inputs < 2p
                    if (j > 1) wb = Tw.ld(i << (r - j - 1));                    // stages 1, 2: i = 0, so w_4^0 = 1 as well
                    wc = Tw.ld((i + half) << (r - j - 1));
                }
                fe x0 = L.ld(l0), x1 = L.ld(l1), x2 = L.ld(l2), x3 = L.ld(l3);
                if (has_wa) { x1 = fe_mul_lazy(x1, wa); x3 = fe_mul_lazy(x3, wa); }
                fe a0 = fe_add_raw(x0, x1), a1 = fe_sub_add_2p(x0, x1), a2 = fe_add_raw(x2, x3), a3 = fe_sub_add_2p(x2, x3);
                a3 = fe_mul_lazy(a3, wc);
                fe y0, y2;
                if (has_wa) { a2 = fe_mul_lazy(a2, wb); y0 = fe_add_raw(a0, a2); y2 = fe_sub_add_2p(a0, a2); }
                else { y0 = fe_add_raw(a0, a2); y2 = fe_sub_add_kp(a0, a2, 4u); }   // a2 = x2 + x3 < 4p unmultiplied: bias 4p, outputs < 8p
                                                                                    // (2p above the usual bound: 20p after ten stages, still < 32p)
                const fe y1 = fe_add_raw(a1, a3), y3 = fe_sub_add_2p(a1, a3);
                if (j + 1 == r && a.radix4 == 1) {
                    if (SP_NTT_PRIO & 2) __builtin_amdgcn_s_setprio(3);
                    // last pair of the pass: straight to global memory (no LDS write, barrier and re-read)
                    const uint32_t q = half;   // = R/4
                    st_fe(m.dst + m.position(t0, gl), a.weak_out ? fe_reduce_lazy_2p(y0) : fe_canonical_lazy(y0));
                    st_fe(m.dst + m.position(t0 + q, gl), a.weak_out ? fe_reduce_lazy_2p(y1) : fe_canonical_lazy(y1));
                    st_fe(m.dst + m.position(t0 + 2 * q, gl), a.weak_out ? fe_reduce_lazy_2p(y2) : fe_canonical_lazy(y2));
                    st_fe(m.dst + m.position(t0 + 3 * q, gl), a.weak_out ? fe_reduce_lazy_2p(y3) : fe_canonical_lazy(y3));
                } else {
                    L.st(l0, y0); L.st(l2, y2); L.st(l1, y1); L.st(l3, y3);
                }
            }
            if (j + 1 != r || a.radix4 != 1) __syncthreads();
        }
        if (a.radix4 == 1) return;   // the last pair has written the tile
    }

    // ------------------------------------------------------------------ store
    store_tile(a, m, tid, L);
}

// table[e] = w^e for e < count, from w^(2^i) (i < bits)
struct RootGenArgs { fe pw[32]; };
__global__ void gen_roots_kernel(fe* table, uint32_t count, uint32_t bits, RootGenArgs args) {
    uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    fe acc = fe_one();
    for (uint32_t i = 0; i < bits; ++i)
        if ((e >> i) & 1) acc = fe_mul(acc, args.pw[i]);
    st_fe(table + e, acc);
}

// data[i] *= base^i * c
struct PowArgs { fe pw[40]; fe c; uint32_t has_c; };
__global__ void scale_powers_kernel(fe* data, uint64_t n, uint64_t stride, PowArgs args) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe acc = args.has_c ? args.c : fe_one();
    for (uint32_t b = 0; b < 40; ++b)
        if ((i >> b) & 1) acc = fe_mul(acc, args.pw[b]);
    fe* p = data + (uint64_t)blockIdx.y * stride + i;
    st_fe(p, fe_mul(ld_fe(p), acc));
}

// ---------------------------------------------------------------------------------------------- host side
static const uint8_t TWO_ADIC_ROOT_BE[32] = {0x00, 0x52, 0x82, 0xdb, 0x87, 0x52, 0x9c, 0xfa, 0x3f, 0x04, 0x64, 0x51, 0x9c, 0x8b, 0x0f, 0xa5,
                                             0xad, 0x18, 0x71, 0x48, 0xe1, 0x1a, 0x61, 0x61, 0x60, 0x70, 0x02, 0x4f, 0x42, 0xf8, 0xef, 0x94};

fe host_primitive_root(int k) {
    fe w = fe_from_bytes_be(TWO_ADIC_ROOT_BE);  // order 2^192
    for (int i = k; i < 192; ++i) w = fe_sqr(w);
    return w;
}

NttEngine::~NttEngine() {
    for (auto& kv : roots_) (void)hipFree(kv.second);
    for (fe* p : pyramids_) (void)hipFree(p);
    for (auto& kv : inv_small_) (void)hipFree(kv.second);
    if (d_scalar_) (void)hipFree(d_scalar_);
}

// d[e] = w^e, e < count
static int fill_table(hipStream_t st, fe w, int bits, uint32_t count, fe* d) {
    RootGenArgs args;
    fe cur = w;
    for (int i = 0; i < 32; ++i) { args.pw[i] = cur; cur = fe_sqr(cur); }
    uint32_t blocks = (count + 255) / 256;
    hipLaunchKernelGGL(gen_roots_kernel, dim3(blocks), dim3(256), 0, st, d, count, (uint32_t)bits, args);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}
static int gen_table(hipStream_t st, fe w, int bits, uint32_t count, fe** out) {
    fe* d = nullptr;
    SP_HIP_CHECK(hipMalloc(&d, sizeof(fe) * (size_t)std::max<uint32_t>(count, 1)));
    const int rc = fill_table(st, w, bits, count, d);
    if (rc != SP_OK) { (void)hipFree(d); return rc; }
    *out = d;
    return SP_OK;
}

// One allocation of 2^kp entries holds the tables of every J <= kp (entry 0 = w_1^0 = 1 serves J = 0).  Every table is generated
// from its own root like a stand-alone roots(J): host_primitive_root(J) = host_primitive_root(kp)^(2^(kp-J)) and all entries are
// canonical, so a slice holds the bytes roots(J) always held.  A larger size builds a new pyramid; the smaller ones are kept
// because kernels in flight and the callers' cached roots() pointers still read them.
int NttEngine::stage_tables(int k, const fe** out) {
    *out = nullptr;
    if (!SP_NTT_STAGE_TW || k > 31) return SP_OK;
    if (k > pyramid_log_) {
        const int kp = std::max(k, NTT_TILE_LOG);    // one small pyramid serves all pass-local tables
        fe* d = nullptr;
        if (hipMalloc(&d, sizeof(fe) << kp) != hipSuccess) { (void)hipGetLastError(); return SP_OK; }   // no room: single-table addressing
        int rc = fill_table(stream_, fe_one(), 0, 1, d);
        for (int J = 1; J <= kp && rc == SP_OK; ++J) rc = fill_table(stream_, host_primitive_root(J), J, 1u << (J - 1), d + (1u << (J - 1)));
        if (rc != SP_OK) { (void)hipFree(d); return rc; }
        pyramids_.push_back(d);
        pyramid_log_ = kp;
    }
    *out = pyramids_.back();
    return SP_OK;
}

int NttEngine::roots(int k, const fe** out) {
    auto it = roots_.find(k);
    if (it == roots_.end()) {
        const fe* pyr = nullptr;
        SP_TRY(stage_tables(k, &pyr));
        if (pyr) { *out = pyr + (k == 0 ? 0u : (1u << (k - 1))); return SP_OK; }
        fe* d = nullptr;
        uint32_t count = k == 0 ? 1u : (1u << (k - 1));
        SP_TRY(gen_table(stream_, host_primitive_root(k), k, count, &d));
        it = roots_.emplace(k, d).first;
    }
    *out = it->second;
    return SP_OK;
}

int NttEngine::transform_twiddles(int k, NttPassArgs* a) {
    const fe* pyr = nullptr;
    SP_TRY(stage_tables(k, &pyr));
    a->stage_tw = pyr ? 1u : 0u;
    a->big_tw = pyr;
    if (!pyr) SP_TRY(roots(k, &a->big_tw));
    a->logM = a->logL = (uint32_t)k;
    return SP_OK;
}
int NttEngine::inv_roots_small(int k, const fe** out) {
    auto it = inv_small_.find(k);
    if (it == inv_small_.end()) {
        fe* d = nullptr;
        uint32_t count = k == 0 ? 1u : (1u << (k - 1));
        SP_TRY(gen_table(stream_, fe_inv(host_primitive_root(k)), k, count, &d));
        it = inv_small_.emplace(k, d).first;
    }
    *out = it->second;
    return SP_OK;
}

template <bool DIF, int LM, int SM, bool CONTIG, bool GTW>
static int launch_t(hipStream_t st, const NttPlannedPass& p, const NttPassArgs& a) {
    if ((uint64_t)p.tiles * p.vectors >= (1ull << 31)) { sp_set_error("ntt: batch too large for one launch"); return SP_E_INVALID_ARG; }
    hipLaunchKernelGGL((ntt_pass_kernel<DIF, LM, SM, CONTIG, GTW>), dim3(p.tiles * p.vectors), dim3(NTT_THREADS), p.lds, st, a);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// The instantiation a planned pass names (plan_launch below chose contig and gtw).
int NttEngine::launch_pass(const NttPlannedPass& p, const NttPassArgs& a) {
    const int lm = p.load, sm = p.store;
    if (!p.dif) {
        if (p.contig && p.gtw && lm == NTT_LOAD_INPLACE) return launch_t<false, NTT_LOAD_INPLACE, NTT_STORE_INPLACE, true, true>(stream_, p, a);
        if (p.contig && !p.gtw && lm == NTT_LOAD_INPLACE) return launch_t<false, NTT_LOAD_INPLACE, NTT_STORE_INPLACE, true, false>(stream_, p, a);
        if (p.contig && !p.gtw && lm == NTT_LOAD_GATHER_BITREV) return launch_t<false, NTT_LOAD_GATHER_BITREV, NTT_STORE_INPLACE, true, false>(stream_, p, a);
        if (!p.contig && p.gtw && lm == NTT_LOAD_INPLACE) return launch_t<false, NTT_LOAD_INPLACE, NTT_STORE_INPLACE, false, true>(stream_, p, a);
        if (!p.contig && p.gtw && lm == NTT_LOAD_EXPAND) return launch_t<false, NTT_LOAD_EXPAND, NTT_STORE_INPLACE, false, true>(stream_, p, a);
    } else if (lm == NTT_LOAD_INPLACE) {
        if (p.contig && !p.gtw && sm == NTT_STORE_INPLACE) return launch_t<true, NTT_LOAD_INPLACE, NTT_STORE_INPLACE, true, false>(stream_, p, a);
        if (p.contig && !p.gtw && sm == NTT_STORE_SCATTER_BITREV) return launch_t<true, NTT_LOAD_INPLACE, NTT_STORE_SCATTER_BITREV, true, false>(stream_, p, a);
        if (!p.contig && p.gtw && sm == NTT_STORE_INPLACE) return launch_t<true, NTT_LOAD_INPLACE, NTT_STORE_INPLACE, false, true>(stream_, p, a);
    }
    sp_set_error("ntt: unsupported pass mode");
    return SP_E_UNSUPPORTED;
}

// Builds the pass list for a size-2^k transform. first_contig_max limits the s = 0 pass (gather/scatter passes
// want G >= 4 rows per tile so that their strided side is coalesced).
struct PassGeom { int s, r, g; };
// footprint = bytes the whole batched transform touches.  1024-element tiles (256-byte rows; the only ones that run their
// stages in pairs) for everything beyond 64 MB, 512-element tiles (more work-groups in flight) for small transforms.
// Measured with the pair kernels: single 2^22 transform 0.383 -> 0.371 ms with 1024, single 2^20 0.114 -> 0.117 ms.
static std::vector<PassGeom> geometry(int k, int first_stride_log, int first_contig_max, uint64_t footprint) {
    const int min_tile_log = footprint > (64ull << 20) ? 10 : 9;
    std::vector<PassGeom> out;
    int s = first_stride_log;
    int rem = k - first_stride_log;
    if (rem <= 0) return out;
    if (s == 0) {
        int r1 = std::min(rem, first_contig_max);
        int g = std::min(NTT_TILE_LOG - r1, k - r1);
        out.push_back({0, r1, g});
        s = r1; rem -= r1;
    }
    if (rem > 0) {
        int np = (rem + NTT_MAX_STRIDED_LOG - 1) / NTT_MAX_STRIDED_LOG;
        std::vector<int> takes;
        for (int i = 0, left = rem; i < np; ++i) { int take = (left + (np - i) - 1) / (np - i); takes.push_back(take); left -= take; }
        if (SP_NTT_EVEN_SPLIT)   // trade stages between two odd passes where the tile allows it (top of the file)
            for (size_t i = 0; i < takes.size(); ++i)
                for (size_t j = i + 1; j < takes.size(); ++j)
                    if ((takes[i] & 1) && (takes[j] & 1) && takes[i] + 1 <= NTT_MAX_STRIDED_LOG && takes[j] >= 3) { takes[i] += 1; takes[j] -= 1; }
        for (int take : takes) {
            // adjacent elements per row: at least 4 (128 B), more for short passes so that a tile never has fewer
            // than 2^min_tile_log elements (a 2^5-row pass with 4 columns would leave half the work-group idle)
            int g = std::min(std::max(NTT_STRIDED_G_LOG, min_tile_log - take), s);
            out.push_back({s, take, g});
            s += take;
        }
    }
    return out;
}
// The passes of a size-2^k transform that starts with a contiguous pass: one tile takes all of it, beyond that the contiguous
// pass has at most 2^contig_cap rows.  k = 0 is one pass without stages (it still loads, scales and stores).
static std::vector<PassGeom> transform_geometry(int k, int contig_cap, uint64_t vectors) {
    std::vector<PassGeom> geo = geometry(k, 0, k <= NTT_TILE_LOG ? NTT_TILE_LOG : contig_cap, (vectors << k) * sizeof(fe));
    if (geo.empty()) geo.push_back({0, 0, 0});
    return geo;
}

// What launching one pass of local (s, r, g) on arrays of 2^logL elements comes to: the kernel variant, tiles, LDS, pairs, XCD order.
// A contiguous pass reads the pass-local table unless it runs the cosets of the coset-major LDE, whose twiddles carry the coset index
// (the transform's table, GTW); strided passes - the EXPAND pass even at local stride 0 - always read the transform's table.
static NttPlannedPass plan_launch(bool dif, int load, int store, const PassGeom& g, uint32_t logL, uint32_t vectors, uint32_t coset_count) {
    NttPlannedPass p{};
    p.dif = dif; p.load = load; p.store = store;
    p.s = (uint32_t)g.s; p.r = (uint32_t)g.r; p.g = (uint32_t)g.g;
    p.logL = logL; p.vectors = vectors; p.coset_count = coset_count;
    p.contig = g.s == 0 && load != NTT_LOAD_EXPAND;
    p.gtw = !p.contig || (!dif && coset_count != 0);
    const uint32_t tile_log = p.r + p.g;
    p.tiles = 1u << (logL - tile_log);
    p.xcd_map = (p.tiles % 8 == 0) ? 1u : 0u;
    // two stages per LDS round trip on the tiles that give every thread a unit (a half-empty work-group loses more than the
    // saved round trips)
    p.radix4 = (p.r >= 2 && (1u << tile_log) == 4u * NTT_THREADS) ? 1u : 0u;
    p.lds = ((size_t)2 << tile_log) * sizeof(uint4) + ((size_t)1 << p.r) * sizeof(uint4);
    if (!p.contig) p.lds = ((size_t)3 << tile_log) * sizeof(uint4);   // tile + the global twiddles of its stages j < r (j < r - 1 in pairs, below)
    else if (p.gtw) p.lds = ((size_t)2 << tile_log) * sizeof(uint4) + ((size_t)2 << p.r) * sizeof(uint4);
    if (!p.contig && p.radix4) p.lds = ((size_t)5 << (tile_log - 1)) * sizeof(uint4);
    return p;
}

std::vector<NttPlannedPass> ntt_plan(NttDriver drv, int k, int logb, int shard_log, uint32_t batch) {
    std::vector<PassGeom> geo;
    bool dif = false;
    int first_load = NTT_LOAD_INPLACE, last_store = NTT_STORE_INPLACE;
    uint32_t logL = (uint32_t)k, vectors = batch, coset_count = 0, stage_tw = (SP_NTT_STAGE_TW && k <= 31) ? 1u : 0u;
    switch (drv) {
        case NTT_DRV_FORWARD_NATURAL:
            geo = transform_geometry(k, NTT_TILE_LOG - NTT_STRIDED_G_LOG, batch);
            first_load = NTT_LOAD_GATHER_BITREV;
            break;
        case NTT_DRV_INVERSE_NATURAL:
            geo = transform_geometry(k, NTT_TILE_LOG - NTT_STRIDED_G_LOG, batch);
            dif = true; last_store = NTT_STORE_SCATTER_BITREV;
            break;
        case NTT_DRV_DIT_BITREV_TO_NATURAL:
            if (k == 0) return {};
            geo = transform_geometry(k, NTT_MAX_CONTIG_LOG, batch);
            break;
        case NTT_DRV_DIF_NATURAL_TO_BITREV_INVERSE: {
            // beyond one tile the contiguous pass is kept short (2^7 rows x 8 contiguous runs): a 2^10-row pass stages a 16 KB
            // twiddle table per 32 KB tile and fits only three work-groups per CU (measured 55 % of the strided passes' rate)
            constexpr int contig_cap = 7;
            geo = transform_geometry(k, contig_cap, batch);
            dif = true;
            break;
        }
        case NTT_DRV_LDE_FROM_BITREV: {
            if (logb == 0) return ntt_plan(NTT_DRV_DIT_BITREV_TO_NATURAL, k, 0, 0, batch);   // plain evaluation: copy, then the DIT in place
            const int K = k + logb;
            geo = geometry(K, logb, NTT_MAX_CONTIG_LOG, ((uint64_t)batch << (K - shard_log)) * sizeof(fe));
            if (geo.empty()) geo.push_back({logb, 0, std::min(logb, NTT_STRIDED_G_LOG)});   // k == 0: constant polynomial replicated
            for (PassGeom& g : geo) {
                g.s -= shard_log;               // local stride
                g.g = std::min(g.g, g.s);       // adjacent elements per row cannot exceed the local stride
            }
            logL = (uint32_t)(K - shard_log); first_load = NTT_LOAD_EXPAND; stage_tw = 0;
            break;
        }
        case NTT_DRV_LDE_COSET_MAJOR:
            coset_count = 1u << (logb - shard_log);
            vectors = batch * coset_count;
            geo = transform_geometry(k, NTT_TILE_LOG - NTT_STRIDED_G_LOG, (uint64_t)batch * coset_count);
            stage_tw = 0;
            break;
    }
    // DIT runs the list first to last, DIF last to first
    std::vector<NttPlannedPass> plan;
    for (size_t step = 0; step < geo.size(); ++step) {
        const bool last = step + 1 == geo.size();
        NttPlannedPass p = plan_launch(dif, step == 0 ? first_load : NTT_LOAD_INPLACE, last ? last_store : NTT_STORE_INPLACE,
                                       geo[dif ? geo.size() - 1 - step : step], logL, vectors, coset_count);
        p.weak_out = !last;
        p.stage_tw = stage_tw;
        plan.push_back(p);
    }
    return plan;
}

// One pass as a driver's hook sees it: the runner has filled what the plan says, the hook names the buffers.
struct NttEngine::PassJob {
    NttPassArgs a;
    void io(const fe* src, fe* dst, uint64_t src_stride, uint64_t dst_stride) { a.src = src; a.dst = dst; a.src_vec_stride = src_stride; a.dst_vec_stride = dst_stride; }
};
// Runs the passes of `plan` in order (the inverse pass-local tables for DIF).  `common` carries what all passes share (twiddle
// source, logM, logL, shifts, coset fields); hook(step, last, job) sees every pass in execution order.
template <class Hook>
int NttEngine::run_passes(const std::vector<NttPlannedPass>& plan, const NttPassArgs& common, Hook hook) {
    for (size_t step = 0; step < plan.size(); ++step) {
        const NttPlannedPass& p = plan[step];
        const bool last = step + 1 == plan.size();
        PassJob job{common};
        job.a.s = p.s; job.a.r = p.r; job.a.g = p.g;
        SP_TRY(p.dif ? inv_roots_small((int)p.r, &job.a.small_tw) : roots((int)p.r, &job.a.small_tw));
        job.a.weak_out = p.weak_out; job.a.radix4 = p.radix4; job.a.xcd_map = p.xcd_map; job.a.batch = p.vectors;
        job.a.stage_tw = (p.stage_tw && common.stage_tw) ? 1u : 0u;   // (the plan assumes the pyramid; transform_twiddles knows whether it is there)
        hook(step, last, job);
        SP_TRY(launch_pass(p, job.a));
    }
    return SP_OK;
}

int NttEngine::dit_bitrev_to_natural(fe* data, int k, uint32_t batch, uint64_t stride) {
    if (k == 0) return SP_OK;
    NttPassArgs c{};
    SP_TRY(transform_twiddles(k, &c));
    return run_passes(ntt_plan(NTT_DRV_DIT_BITREV_TO_NATURAL, k, 0, 0, batch), c,
                      [&](size_t, bool, PassJob& j) { j.io(data, data, stride, stride); });
}

int NttEngine::dif_natural_to_bitrev_inverse(fe* data, int k, uint32_t batch, uint64_t stride, const fe* post_table, const fe* src) {
    NttPassArgs c{};
    SP_TRY(transform_twiddles(k, &c));
    return run_passes(ntt_plan(NTT_DRV_DIF_NATURAL_TO_BITREV_INVERSE, k, 0, 0, batch), c, [&](size_t step, bool last, PassJob& j) {
        j.io(src && step == 0 ? src : data, data, stride, stride);   // the first pass executed may read another array (same stride)
        if (last) j.a.post_table = post_table;
    });
}

int NttEngine::forward_natural(const fe* src, fe* dst, int k, uint32_t batch, uint64_t ss, uint64_t ds, fe* final_dst) {
    NttPassArgs c{};
    SP_TRY(transform_twiddles(k, &c));
    const std::vector<NttPlannedPass> plan = ntt_plan(NTT_DRV_FORWARD_NATURAL, k, 0, 0, batch);
    // ping-pong: pass 1 src -> dst (gather, must be out of place); if final_dst is given (same stride as src), pass 2
    // writes dst -> final_dst and later passes run in place there, so the result lands in final_dst without a copy.
    fe* const rest = final_dst ? final_dst : dst;
    const uint64_t rs = final_dst ? ss : ds;
    SP_TRY(run_passes(plan, c, [&](size_t step, bool, PassJob& j) {
        if (step == 0) j.io(src, dst, ss, ds);
        else if (step == 1) j.io(dst, rest, ds, rs);
        else j.io(rest, rest, rs, rs);
    }));
    if (final_dst && plan.size() == 1)
        for (uint32_t v = 0; v < batch; ++v)
            SP_HIP_CHECK(hipMemcpyAsync(final_dst + v * ss, dst + v * ds, sizeof(fe) << k, hipMemcpyDeviceToDevice, stream_));
    return SP_OK;
}

int NttEngine::inverse_natural(fe* data, fe* tmp, int k, uint32_t batch, uint64_t stride) {
    // Un-passes run last-to-first: the first one goes data -> tmp, the middle ones stay in tmp, and the final
    // bit-reversal scatter goes tmp -> data (a scatter must never run in place: other tiles still read their rows).
    NttPassArgs c{};
    SP_TRY(transform_twiddles(k, &c));
    const std::vector<NttPlannedPass> plan = ntt_plan(NTT_DRV_INVERSE_NATURAL, k, 0, 0, batch);
    if (!d_scalar_) SP_HIP_CHECK(hipMalloc(&d_scalar_, sizeof(fe)));
    fe ninv = fe_inv(fe_from_u64(1ULL << k));
    SP_HIP_CHECK(hipMemcpyAsync(d_scalar_, &ninv, sizeof(fe), hipMemcpyHostToDevice, stream_));
    const bool one_pass = plan.size() == 1;
    if (one_pass) {
        for (uint32_t v = 0; v < batch; ++v)
            SP_HIP_CHECK(hipMemcpyAsync(tmp + v * stride, data + v * stride, sizeof(fe) << k, hipMemcpyDeviceToDevice, stream_));
    }
    return run_passes(plan, c, [&](size_t step, bool last, PassJob& j) {
        j.io(step == 0 && !one_pass ? data : tmp, last ? data : tmp, stride, stride);
        if (last) j.a.scalar = d_scalar_;
    });
}

int NttEngine::lde_from_bitrev(const fe* coeffs, fe* dst, int k, int logb, uint32_t batch, uint64_t ss, uint64_t ds,
                               int shard_log, int shard_rank) {
    int K = k + logb;
    if (shard_log < 0 || shard_log > logb) { sp_set_error("lde: more shards than cosets"); return SP_E_INVALID_ARG; }
    if (logb == 0) {  // plain evaluation: copy then DIT in place
        for (uint32_t v = 0; v < batch; ++v)
            SP_HIP_CHECK(hipMemcpyAsync(dst + v * ds, coeffs + v * ss, sizeof(fe) << k, hipMemcpyDeviceToDevice, stream_));
        return dit_bitrev_to_natural(dst, k, batch, ds);
    }
    NttPassArgs c{};
    SP_TRY(roots(K, &c.big_tw));
    c.logM = K; c.logL = (uint32_t)(K - shard_log); c.log_expand = logb;
    c.tw_shift = (uint32_t)shard_log; c.tw_low = (uint32_t)shard_rank;   // local index -> global: (index << shard_log) | rank
    return run_passes(ntt_plan(NTT_DRV_LDE_FROM_BITREV, k, logb, shard_log, batch), c, [&](size_t step, bool, PassJob& j) {
        if (step == 0) j.io(coeffs, dst, ss, ds);
        else j.io(dst, dst, ds, ds);
    });
}

// Coset-major LDE: dst column v = [coset c_loc][m], element = p_v(h w_N^(m b + c)) with c = c_loc * 2^shard_log + rank.
// Every coset is a size-n DIT of the same bit-reversed coefficients whose twiddles carry the coset index in their low
// bits (w_N^(((m mod 2^(j-1)) b + c) << (K - logb - j)) at stage j): the first pass is a contiguous one (coalesced
// reads of the coefficients, no replication), and what consumes one or two cosets - the constraint composition, the
// DEEP quotient - reads contiguous memory instead of every b-th or (b/2)-th element of the natural order.
int NttEngine::lde_coset_major(const fe* coeffs, fe* dst, int k, int logb, uint32_t batch, uint64_t ss, uint64_t ds, int shard_log, int shard_rank) {
    const int K = k + logb;
    if (shard_log < 0 || shard_log > logb) { sp_set_error("lde: more shards than cosets"); return SP_E_INVALID_ARG; }
    const uint32_t b_loc = 1u << (logb - shard_log);
    const uint64_t n = 1ull << k;
    NttPassArgs c{};
    SP_TRY(roots(K, &c.big_tw));
    c.logM = K; c.logL = (uint32_t)k;
    c.tw_shift = (uint32_t)logb; c.tw_low = (uint32_t)shard_rank; c.shard_log = (uint32_t)shard_log;
    c.coset_count = b_loc; c.dst_coset_stride = n;
    return run_passes(ntt_plan(NTT_DRV_LDE_COSET_MAJOR, k, logb, shard_log, batch), c, [&](size_t step, bool, PassJob& j) {
        if (step == 0) j.io(coeffs, dst, ss, ds);          // every coset reads the same coefficients
        else { j.io(dst, dst, ds, ds); j.a.src_coset_stride = n; }
    });
}

int NttEngine::scale_by_powers(fe* data, uint64_t n, uint32_t batch, uint64_t stride, const fe& base, const fe* c) {
    PowArgs args;
    fe cur = base;
    for (int i = 0; i < 40; ++i) { args.pw[i] = cur; cur = fe_sqr(cur); }
    args.has_c = c ? 1 : 0;
    args.c = c ? *c : fe_one();
    dim3 grid((unsigned)((n + 255) / 256), batch);
    hipLaunchKernelGGL(scale_powers_kernel, grid, dim3(256), 0, stream_, data, n, stride, args);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

}  // namespace sp
