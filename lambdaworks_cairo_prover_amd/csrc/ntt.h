// Stark252 NTT engine for gfx950: multi-stage passes through LDS, radix-2 stages inside a pass.
//
// Replaces the lambdaworks FFTPoly calls of the reference: Polynomial::interpolate_fft (src/starks/trace.rs:107),
// interpolate_offset_fft (src/starks/constraints/evaluation_table.rs:32), evaluate_offset_fft
// (src/starks/prover.rs:117, src/starks/fri/fri_commitment.rs:36).
//
// A size-2^k transform is a chain of passes; each pass runs r consecutive radix-2 stages of the plain in-place algorithm
// (Cooley-Tukey DIT: bit-reversed in -> natural out; Gentleman-Sande DIF: natural in -> bit-reversed out) on tiles staged
// in LDS.  The s = 0 pass works on contiguous tiles, the others on tiles of R = 2^r rows at stride 2^s x G adjacent
// elements (G*32 B contiguous per row -> coalesced) together with the twiddles of exactly those butterflies.
// All memory orders are chosen so the prover never needs a bit-reversal pass: iNTT leaves coefficients
// bit-reversed, the LDE consumes them bit-reversed and emits natural order.
//
// ntt.hip, device side: ntt_pass_kernel<DIF, LOADM, STOREM, CONTIG, GTW> runs tile map, twiddles, load | stages | store.
// TileMap maps the block id to tile and vector (XCD order, the coset-major split) and a tile element to its position() in
// memory and its lidx() in LDS; LdsPlanes is the tile or the twiddle table in LDS; global_tw() addresses the transform's
// table; load_tile and store_tile move the tile.  The twiddle staging and the stages themselves (radix-4 units of both
// directions, the radix-2 stage, the DIT pass's fused last-pair store) stand in the kernel body.
// Host side: ntt_plan() turns (driver, k, logb, shard_log, batch) into the pass list as it is launched - kernel variant, local
// s / r / g, tile count, LDS bytes, radix4 / xcd_map / weak_out / stage_tw - without touching the device; every driver hands that list,
// the fields all passes share and a per-pass hook (buffers, strides, post_table / scalar on the last pass) to the one pass loop,
// run_passes, which launches exactly what the list says.  sp_ntt_plan (capi_dev.cpp) hands the same list to tests.
#pragma once
#include "common.h"
#include <map>
#include <vector>

namespace sp {

constexpr int NTT_TILE_LOG = 10;                 // elements per workgroup tile (2^10 x 32 B = 32 KiB of LDS)
constexpr int NTT_THREADS = 256;
constexpr int NTT_MAX_CONTIG_LOG = NTT_TILE_LOG; // s = 0 pass: one row of up to 2^10 contiguous elements
constexpr int NTT_STRIDED_G_LOG = 2;             // strided passes: 4 adjacent elements (128 B) per row
constexpr int NTT_MAX_STRIDED_LOG = NTT_TILE_LOG - NTT_STRIDED_G_LOG;

struct NttPassArgs {
    const fe* src;
    fe* dst;
    uint64_t src_vec_stride, dst_vec_stride;  // elements between consecutive vectors of the batch
    const fe* small_tw;   // s = 0 pass: w_R^(+-e), e in [0, R/2)   (direction chosen by the host)
    const fe* big_tw;     // strided passes: w_M^e, e in [0, M/2)  (forward roots; the inverse butterfly uses w^-e = -w^(M/2-e));
                          // with stage_tw the engine's pyramid of per-stage tables: w_(2^J)^x at entry 2^(J-1) + x, x < 2^(J-1)
    const fe* post_table; // DIF only, nullable: multiply the element stored at position pos by post_table[pos]
    const fe* scalar;     // nullable: multiply every stored element by *scalar (device pointer)
    uint32_t logM;        // transform size (twiddles are powers of w_(2^logM))
    uint32_t logL;        // log2 of the array this pass addresses (per vector, per coset in the coset-major LDE)
    uint32_t s, r, g;     // this pass: LOCAL stride 2^s, R = 2^r rows, G = 2^g adjacent elements per row
    uint32_t log_expand;  // EXPAND load: src index = pos >> s on the first pass (zero-padded/replicated LDE input)
    // Local index -> index of the size-2^logM transform: (local << tw_shift) | tw_low.  tw_shift = 0 for whole transforms;
    // natural-order LDE sharded over 2^shard ranks: tw_shift = shard, tw_low = rank (this rank holds the cosets
    // c = c_loc * 2^shard + rank interleaved); coset-major LDE: tw_shift = log2(blowup), tw_low = the coset's global index.
    uint32_t tw_shift, tw_low;
    // coset-major LDE: launch "vector" = column * coset_count + local coset; arrays at column * vec_stride + coset * coset_stride;
    // the global coset index is (local coset << shard_log) | tw_low.  coset_count = 0: plain vectors.
    uint32_t coset_count, shard_log;
    uint64_t src_coset_stride, dst_coset_stride;
    // 1 on every pass but the last one of a transform: the stored data is only brought below 2p; 0: canonical values.
    uint32_t weak_out;
    uint32_t stage_tw;    // 1: big_tw is the pyramid, stage J reads its own dense table (adjacent columns = adjacent entries)
    uint32_t radix4;      // two stages per LDS round trip (from the plan)
    uint32_t batch;       // vectors per launch (from the plan)
    uint32_t xcd_map;     // 1: XCD-aware block -> (tile, vector) mapping (needs tiles % 8 == 0)
};

enum NttLoadMode { NTT_LOAD_INPLACE = 0, NTT_LOAD_GATHER_BITREV = 1, NTT_LOAD_EXPAND = 2 };
enum NttStoreMode { NTT_STORE_INPLACE = 0, NTT_STORE_SCATTER_BITREV = 1 };

// The six drivers of the engine, as ntt_plan and sp_ntt_plan name them (the values are the SP_NTT_DRIVER_* of the C header).
enum NttDriver { NTT_DRV_FORWARD_NATURAL = 0, NTT_DRV_INVERSE_NATURAL = 1, NTT_DRV_DIT_BITREV_TO_NATURAL = 2,
                 NTT_DRV_DIF_NATURAL_TO_BITREV_INVERSE = 3, NTT_DRV_LDE_FROM_BITREV = 4, NTT_DRV_LDE_COSET_MAJOR = 5 };
// One launch of ntt_pass_kernel as a driver will make it, in execution order.
struct NttPlannedPass {
    bool dif;                 // Gentleman-Sande (inverse roots) or Cooley-Tukey
    int load, store;          // NttLoadMode, NttStoreMode
    bool contig, gtw;         // template flags CONTIG and GTW of the instantiation
    uint32_t s, r, g;         // LOCAL stride 2^s, 2^r rows, 2^g adjacent elements per row
    uint32_t radix4, xcd_map, weak_out;
    uint32_t stage_tw;        // 1: reads the pyramid of per-stage tables when the engine has one (whole transforms of a -DSP_NTT_STAGE_TW=1 build)
    uint32_t logL;            // log2 of the array the pass addresses (per vector, per coset in the coset-major LDE)
    uint32_t tiles;           // work-groups per vector
    uint32_t vectors;         // vectors per launch (columns x local cosets in the coset-major LDE)
    uint32_t coset_count;     // coset-major LDE: local cosets per column; 0: plain vectors
    size_t lds;               // dynamic LDS bytes of the launch
};
// The passes driver `drv` launches for 2^k elements per vector, blowup 2^logb, 2^shard_log shards and `batch` vectors (logb and
// shard_log count for the two LDE drivers only).  Pure host arithmetic: no device, no engine.
std::vector<NttPlannedPass> ntt_plan(NttDriver drv, int k, int logb, int shard_log, uint32_t batch);

class NttEngine {
  public:
    explicit NttEngine(hipStream_t stream) : stream_(stream) {}
    ~NttEngine();
    // device table w_(2^k)^e, e in [0, 2^(k-1)); cached per k (a slice of the pyramid below where one covers k).  The pointer
    // stays valid until the engine is destroyed.
    int roots(int k, const fe** out);
    // Pyramid of per-stage twiddle tables covering every stage J <= k: entry 2^(J-1) + x = w_(2^J)^x, x < 2^(J-1) (2^k' entries for
    // some k' >= k; the slice at 2^(J-1) is roots(J)).  *out = nullptr when the device has no room for it: the transforms then
    // address the single table roots(k) with a stride, as they do when built with -DSP_NTT_STAGE_TW=0.
    int stage_tables(int k, const fe** out);
    // device table w_(2^k)^(-e), e in [0, 2^(k-1)); only for small k (pass twiddles)
    int inv_roots_small(int k, const fe** out);

    // bit-reversed input -> natural output, forward roots, in place.  batch vectors at `stride` elements.
    int dit_bitrev_to_natural(fe* data, int k, uint32_t batch, uint64_t stride);
    // natural input -> bit-reversed output, inverse roots, UNSCALED (x 2^k), in place;
    // post_table (nullable, device, 2^k entries indexed by output position) multiplies the result.
    // src (nullable): read the input from another array with the same layout and leave it untouched.
    int dif_natural_to_bitrev_inverse(fe* data, int k, uint32_t batch, uint64_t stride, const fe* post_table, const fe* src = nullptr);
    // natural -> natural forward DFT (evaluate_fft), out of place (src != dst).
    int forward_natural(const fe* src, fe* dst, int k, uint32_t batch, uint64_t src_stride, uint64_t dst_stride, fe* final_dst = nullptr);
    // natural -> natural inverse DFT including the 1/2^k factor (interpolate_fft); result in `data`, tmp = same-size scratch.
    int inverse_natural(fe* data, fe* tmp, int k, uint32_t batch, uint64_t stride);
    // LDE: coeffs = n = 2^k "h-scaled" coefficients (c_j h^j) in bit-reversed order; dst = N = n*2^logb natural-order
    // evaluations p(h w_N^i).  (zero-padded size-N DIT whose first log2(b) stages are replication.)
    // shard_log/shard_rank: compute only the cosets c = c_loc * 2^shard_log + shard_rank (dst holds n * 2^(logb - shard_log)
    // elements per vector, element (q, c_loc) at q * 2^(logb - shard_log) + c_loc).
    int lde_from_bitrev(const fe* coeffs, fe* dst, int k, int logb, uint32_t batch, uint64_t src_stride, uint64_t dst_stride,
                        int shard_log = 0, int shard_rank = 0);
    // The same evaluations in COSET-MAJOR order: dst column v holds 2^(logb - shard_log) arrays of n elements, array c_loc =
    // the coset c = c_loc * 2^shard_log + shard_rank, element m = p(h w_N^(m b + c))  (natural-order index m b + c).
    int lde_coset_major(const fe* coeffs, fe* dst, int k, int logb, uint32_t batch, uint64_t src_stride, uint64_t dst_stride,
                        int shard_log = 0, int shard_rank = 0);

    // dst[i] = src[i] * base^i * c  (natural index), c nullable. Used by the coset variants of sp_ntt.
    int scale_by_powers(fe* data, uint64_t n, uint32_t batch, uint64_t stride, const fe& base, const fe* c);

    hipStream_t stream() const { return stream_; }

  private:
    int launch_pass(const NttPlannedPass& p, const NttPassArgs& a);
    // The one pass loop behind the six drivers above (ntt.hip): walks an ntt_plan() list, fills what follows from the list (s, r, g, the
    // pass-local table of the direction, weak_out, radix4, xcd_map, the launch's vector count) and lets the driver's hook name buffers and strides.
    struct PassJob;
    template <class Hook>
    int run_passes(const std::vector<NttPlannedPass>& plan, const NttPassArgs& common, Hook hook);
    hipStream_t stream_;
    // what the passes of a whole size-2^k transform share: logM = logL = k and the twiddles, pyramid + stage_tw = 1 or roots(k) + stage_tw = 0
    int transform_twiddles(int k, NttPassArgs* a);
    std::map<int, fe*> roots_;       // stand-alone tables (no pyramid covered k and none could be allocated)
    std::vector<fe*> pyramids_;      // the last one is the largest; older ones stay alive for kernels in flight and cached roots()
    int pyramid_log_ = -1;
    std::map<int, fe*> inv_small_;
    fe* d_scalar_ = nullptr;
};

// host helpers
fe host_primitive_root(int k);          // w of order 2^k (lambdaworks get_primitive_root_of_unity)

}  // namespace sp
