// C ABI: context and the fine-grained device entry points (sp_ntt, sp_lde, sp_merkle_build, sp_batch_inverse).
// See include/stark252_hip.h for the reference call sites each one replaces.
#include "ctx.h"
#include "cairo_host.h"
#include <rccl/rccl.h>
#include <chrono>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <vector>

// prover.cpp: the periodic-column tables of a program AIR (sp_air_periodic_lde hands one out)
namespace sp { int air_periodic_tables(hipStream_t st, NttEngine& ntt, fe* vals, fe* ws, fe* tab, uint32_t cnt, uint32_t logp, uint32_t logn, uint32_t logb, const fe& h); }
// prover_round2.cpp: the tables of one stride class (sp_air_stride_table hands out their inverse half)
namespace sp { int air_stride_class_tables(hipStream_t st, NttEngine& ntt, fe* u, fe* z, uint32_t logs, uint32_t offset, uint32_t logn, uint32_t logb, const fe& h); }
using namespace sp;

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) {
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { sp_set_error("hipMalloc failed (" + std::to_string(bytes) + " bytes)"); p = nullptr; return SP_E_ALLOC; }
        return SP_OK;
    }
    template <class T> T* as() { return reinterpret_cast<T*>(p); }
};
}  // namespace

extern "C" {

int sp_device_count(int* count_out) {
    if (!count_out) return SP_E_INVALID_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count_out = n;
    return SP_OK;
}

int sp_ctx_create(sp_ctx** out, const sp_config* cfg) {
    if (!out || !cfg) return SP_E_INVALID_ARG;
    if (cfg->fe_encoding != SP_FE_MONT_LIMBS && cfg->fe_encoding != SP_FE_CANON_BE) return SP_E_INVALID_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { sp_set_error("no HIP device visible: the stark252 HIP path requires an MI355X (gfx950)"); return SP_E_NO_DEVICE; }
    if (cfg->device < 0 || cfg->device >= n) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(cfg->device));
    sp_ctx* c = new sp_ctx();
    c->device = cfg->device;
    c->enc = cfg->fe_encoding;
    if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; sp_set_error("hipStreamCreate failed"); return SP_E_HIP; }
    c->ntt = new NttEngine(c->stream);
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->tev0) != hipSuccess || hipEventCreate(&c->tev1) != hipSuccess) { sp_ctx_destroy(c); return SP_E_HIP; }
    if (hipMalloc(&c->d_flag, sizeof(int)) != hipSuccess) { sp_ctx_destroy(c); return SP_E_ALLOC; }
    if (hipMalloc(&c->d_agree, sp_ctx::kAgreeBytes) != hipSuccess) { sp_ctx_destroy(c); return SP_E_ALLOC; }
    sp::hip_runtime_mark_in_use();
    *out = c;
    return SP_OK;
}

void sp_ctx_destroy(sp_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c->prover_state_deleter_holder;
    delete c->comm_holder;
    delete c->ntt;
    for (hipEvent_t e : c->comm_ev) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->tev0) (void)hipEventDestroy(c->tev0);
    if (c->tev1) (void)hipEventDestroy(c->tev1);
    if (c->d_flag) (void)hipFree(c->d_flag);
    if (c->d_agree) (void)hipFree(c->d_agree);
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int sp_set_collective(sp_ctx* c, int world, int rank, sp_allgather_fn fn, void* user) {
    if (!c || world < 1 || rank < 0 || rank >= world || (world & (world - 1)) || (world > 1 && !fn)) return SP_E_INVALID_ARG;
    if (world != c->world) {                 // a prover shaped for another world size must not survive; for another RANK of the same world
        delete c->prover_state_deleter_holder;   // setup() re-carves the arena it already has (the replayed ranks of tools/replay_ranks.py)
        c->prover_state_deleter_holder = nullptr;
    }
    c->world = world; c->rank = rank; c->allgather = fn; c->allgather_user = user; c->alltoall = nullptr; c->allgather_async = nullptr; c->alltoall_async = nullptr;
    c->comm_is_null = false;
    return SP_OK;
}

int sp_set_collective_async(sp_ctx* c, sp_allgather_async_fn fn) {
    if (!c) return SP_E_INVALID_ARG;
    c->allgather_async = fn;
    return SP_OK;
}

int sp_set_alltoall_async(sp_ctx* c, sp_alltoall_async_fn fn) {
    if (!c) return SP_E_INVALID_ARG;
    c->alltoall_async = fn;
    return SP_OK;
}

int sp_set_alltoall(sp_ctx* c, sp_alltoall_fn fn) {
    if (!c) return SP_E_INVALID_ARG;
    c->alltoall = fn;
    return SP_OK;
}

// Time the collectives of this context took since creation: out[0] the stream-ordered ones (event pairs on the streams they were
// enqueued on: what each exchange occupied its stream for, the wait for the slowest peer included), out[1] the blocking ones (wall
// clock around the hook).  Waits for the context's streams (the events of a proof that has returned are complete anyway).
int sp_comm_time_ms(sp_ctx* c, double out[2]) {
    if (!c || !out) return SP_E_INVALID_ARG;
    if (c->comm_ev_used) {
        SP_HIP_CHECK(hipSetDevice(c->device));
        SP_HIP_CHECK(hipDeviceSynchronize());        // (the communication stream of the prover is not the context stream)
        for (size_t i = 0; i + 1 < c->comm_ev_used; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->comm_ev[i], c->comm_ev[i + 1]) == hipSuccess) c->stat_comm_stream_ms += (double)ms;
        }
        c->comm_ev_used = 0;
    }
    out[0] = c->stat_comm_stream_ms; out[1] = c->stat_comm_blocking_ms;
    return SP_OK;
}

int sp_comm_stats(sp_ctx* c, uint64_t out[6]) {
    if (!c || !out) return SP_E_INVALID_ARG;
    out[0] = (uint64_t)c->world; out[1] = c->stat_ag_calls; out[2] = c->stat_ag_bytes;
    out[3] = c->stat_a2a_calls; out[4] = c->stat_a2a_bytes; out[5] = c->stat_recv_bytes;
    return SP_OK;
}

int sp_set_option(sp_ctx* c, int key, int64_t value) {
    if (!c) return SP_E_INVALID_ARG;
    switch (key) {
        case SP_OPT_FRI_SHARD_MIN_LOG:
            if (value < 1 || value > 40) return SP_E_INVALID_ARG;
            c->opt_fri_shard_min_log = (uint32_t)value;
            break;
        case SP_OPT_SHARD_INTERPOLATION:
            if (value < 0 || value > 2) return SP_E_INVALID_ARG;
            c->opt_shard_interpolation = (int)value;
            break;
        case SP_OPT_LINK_GBS:
            if (value < 1 || value > 10000) return SP_E_INVALID_ARG;
            c->opt_link_gbs = (double)value;
            c->opt_link_gbs_explicit = true;      // the caller's word beats a measurement (sp_comm_measure)
            break;
        case SP_OPT_UPLOAD_THREADS:
            if (value < 1 || value > 128) return SP_E_INVALID_ARG;
            c->opt_upload_threads = (uint32_t)value;
            break;
        case SP_OPT_MERKLE_BACKEND:
            if (value != SP_MERKLE_KECCAK256 && value != SP_MERKLE_POSEIDON) return SP_E_INVALID_ARG;
            c->opt_merkle_backend = (int)value;
            break;
        case SP_OPT_HOST_RANKS:
            if (value < 0 || value > 1024) return SP_E_INVALID_ARG;
            sp::set_host_ranks((unsigned)value);      // (process-wide: one context per process and GPU; 0 = back to the environment)
            return SP_OK;                     // (shapes no prover buffer; the gather pool follows at the next upload)
        case SP_OPT_DEVICE_TRACE:
            c->opt_device_trace = value != 0;
            return SP_OK;                     // (shapes no prover buffer)
        case SP_OPT_MERKLE_ONE_COLUMN_ROWS:
            c->opt_merkle_one_column_rows = value != 0;
            return SP_OK;                     // (shapes no prover buffer)
        default: sp_set_error("sp_set_option: unknown key"); return SP_E_INVALID_ARG;
    }
    delete c->prover_state_deleter_holder;   // the options shape the prover's buffers: start from a fresh one
    c->prover_state_deleter_holder = nullptr;
    return SP_OK;
}

namespace {
struct RcclComm : public sp_deletable {
    ncclComm_t comm = nullptr;
    hipStream_t stream = nullptr;
    int world = 1;
    ~RcclComm() override { if (comm) (void)ncclCommDestroy(comm); }
};
int rccl_allgather(void* user, const void* send, void* recv, uint64_t bytes) {
    RcclComm* rc = static_cast<RcclComm*>(user);
    if (ncclAllGather(send, recv, bytes, ncclUint8, rc->comm, rc->stream) != ncclSuccess) return -1;
    if (hipStreamSynchronize(rc->stream) != hipSuccess) return -2;
    return 0;
}
int rccl_allgather_async(void* user, const void* send, void* recv, uint64_t bytes, void* stream) {
    RcclComm* rc = static_cast<RcclComm*>(user);
    return ncclAllGather(send, recv, bytes, ncclUint8, rc->comm, static_cast<hipStream_t>(stream)) == ncclSuccess ? 0 : -1;
}
// all-to-all of equal blocks as grouped point-to-point transfers (xGMI is point-to-point: every pair uses its own link)
int rccl_alltoall_async(void* user, const void* send, void* recv, uint64_t bytes, void* stream) {
    RcclComm* rc = static_cast<RcclComm*>(user);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t* s = static_cast<const uint8_t*>(send);
    uint8_t* r = static_cast<uint8_t*>(recv);
    if (ncclGroupStart() != ncclSuccess) return -1;
    int rcode = 0;   // the group is closed whatever happens inside it: a communicator left in group mode queues every later call
    for (int peer = 0; peer < rc->world && rcode == 0; ++peer) {
        if (ncclSend(s + (size_t)peer * bytes, bytes, ncclUint8, peer, rc->comm, st) != ncclSuccess) rcode = -3;
        else if (ncclRecv(r + (size_t)peer * bytes, bytes, ncclUint8, peer, rc->comm, st) != ncclSuccess) rcode = -4;
    }
    if (ncclGroupEnd() != ncclSuccess && rcode == 0) rcode = -5;
    return rcode;
}
int rccl_alltoall(void* user, const void* send, void* recv, uint64_t bytes) {
    RcclComm* rc = static_cast<RcclComm*>(user);
    const int rcode = rccl_alltoall_async(user, send, recv, bytes, rc->stream);
    if (rcode != 0) return rcode;
    if (hipStreamSynchronize(rc->stream) != hipSuccess) return -2;
    return 0;
}
}  // namespace

namespace {
// Timing-only transport (sp_comm_init_null): nothing is exchanged.  The own block lands where a real collective would put it and
// the blocks of the other ranks are zero-filled - the HBM writes a real receive would cost - so a single GPU can run ONE rank's
// share of a sharded proof with every kernel at its real size.  The proof bytes that come out are meaningless.
struct NullComm : public sp_deletable { hipStream_t stream = nullptr; int world = 1, rank = 0; };
int null_allgather(void* user, const void* send, void* recv, uint64_t bytes) {
    NullComm* nc = static_cast<NullComm*>(user);
    uint8_t* r = static_cast<uint8_t*>(recv);
    uint8_t* mine = r + (size_t)nc->rank * bytes;
    if (mine != send && hipMemcpyAsync(mine, send, bytes, hipMemcpyDeviceToDevice, nc->stream) != hipSuccess) return -1;
    if (nc->rank > 0 && hipMemsetAsync(r, 0, (size_t)nc->rank * bytes, nc->stream) != hipSuccess) return -1;
    if (nc->rank + 1 < nc->world && hipMemsetAsync(mine + bytes, 0, (size_t)(nc->world - 1 - nc->rank) * bytes, nc->stream) != hipSuccess) return -1;
    return hipStreamSynchronize(nc->stream) == hipSuccess ? 0 : -2;
}
int null_allgather_async(void* user, const void* send, void* recv, uint64_t bytes, void* stream) {
    NullComm* nc = static_cast<NullComm*>(user);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* r = static_cast<uint8_t*>(recv);
    uint8_t* mine = r + (size_t)nc->rank * bytes;
    if (mine != send && hipMemcpyAsync(mine, send, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return -1;
    if (nc->rank > 0 && hipMemsetAsync(r, 0, (size_t)nc->rank * bytes, st) != hipSuccess) return -1;
    if (nc->rank + 1 < nc->world && hipMemsetAsync(mine + bytes, 0, (size_t)(nc->world - 1 - nc->rank) * bytes, st) != hipSuccess) return -1;
    return 0;
}
int null_alltoall_async(void* user, const void* send, void* recv, uint64_t bytes, void* stream) {
    NullComm* nc = static_cast<NullComm*>(user);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* r = static_cast<uint8_t*>(recv);
    if (hipMemsetAsync(r, 0, (size_t)nc->world * bytes, st) != hipSuccess) return -1;
    if (hipMemcpyAsync(r + (size_t)nc->rank * bytes, static_cast<const uint8_t*>(send) + (size_t)nc->rank * bytes, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return -1;
    return 0;
}
int null_alltoall(void* user, const void* send, void* recv, uint64_t bytes) {
    NullComm* nc = static_cast<NullComm*>(user);
    if (null_alltoall_async(user, send, recv, bytes, nc->stream) != 0) return -1;
    return hipStreamSynchronize(nc->stream) == hipSuccess ? 0 : -2;
}
}  // namespace

int sp_comm_init_null(sp_ctx* c, int world, int rank) {
    if (!c || world < 1 || rank < 0 || rank >= world || (world & (world - 1))) return SP_E_INVALID_ARG;
    NullComm* nc = new NullComm();
    nc->stream = c->stream; nc->world = world; nc->rank = rank;
    delete c->comm_holder;
    c->comm_holder = nc;
    SP_TRY(sp_set_collective(c, world, rank, null_allgather, nc));
    c->comm_is_null = true;
    SP_TRY(sp_set_collective_async(c, null_allgather_async));
    SP_TRY(sp_set_alltoall_async(c, null_alltoall_async));
    return sp_set_alltoall(c, null_alltoall);
}

int sp_comm_unique_id(uint8_t id_out[128]) {
    if (!id_out) return SP_E_INVALID_ARG;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) { sp_set_error("ncclGetUniqueId failed"); return SP_E_HIP; }
    std::memcpy(id_out, &id, 128);
    return SP_OK;
}

int sp_comm_init_rccl(sp_ctx* c, const uint8_t id_bytes[128], int world, int rank) {
    if (!c || !id_bytes || world < 1 || rank < 0 || rank >= world || (world & (world - 1))) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    ncclUniqueId id;
    std::memcpy(&id, id_bytes, 128);
    RcclComm* rc = new RcclComm();
    rc->stream = c->stream; rc->world = world;
    if (ncclCommInitRank(&rc->comm, world, id, rank) != ncclSuccess) { delete rc; sp_set_error("ncclCommInitRank failed"); return SP_E_HIP; }
    delete c->comm_holder;
    c->comm_holder = rc;
    SP_TRY(sp_set_collective(c, world, rank, rccl_allgather, rc));
    SP_TRY(sp_set_collective_async(c, rccl_allgather_async));
    SP_TRY(sp_set_alltoall_async(c, rccl_alltoall_async));
    SP_TRY(sp_set_alltoall(c, rccl_alltoall));
    // One timed all-gather and all-to-all per communicator (64 MB per rank; SP_COMM_MEASURE_MB, 0 = none): opens RCCL's channels
    // before the first proof needs them, and gives SP_OPT_SHARD_INTERPOLATION = 2 a measured link rate instead of an assumed one.
    uint64_t mb = 64;
    if (const char* e = std::getenv("SP_COMM_MEASURE_MB")) mb = (uint64_t)std::min(1024, std::max(0, std::atoi(e)));
    // A measurement that fails is not a communicator that fails: sp_comm_measure agrees on the outcome across the ranks, so EVERY rank
    // then keeps the assumed rate (zeroed figures) and takes the same interpolation mode (sp_comm_selftest is the functional check).
    if (world > 1 && mb) (void)sp_comm_measure(c, mb << 20, nullptr);
    return SP_OK;
}

// The link model behind SP_OPT_SHARD_INTERPOLATION = 2 as a pure function (unit-tested with injected rates): interpolation by column
// saves a rank (1 - 1/G) of the size-n inverse transforms - n log2(n) / 2 butterflies per column at ~1.35e11 / s - and makes it receive
// (1 - 1/G) of the coefficients, 32 n bytes per column, over G - 1 links: it pays when 64 x 1.35e11 < (G - 1) x link bytes/s x log2 n.
int sp_model_shard_interpolation(double link_gbs_per_direction, uint32_t groups, uint32_t log2_rows) {
    if (groups < 2 || !(link_gbs_per_direction > 0)) return 0;
    return 64.0 * 1.35e11 < (double)(groups - 1) * link_gbs_per_direction * 1e9 * (double)log2_rows ? 1 : 0;
}

// Times the installed transport: all-gathers and all-to-alls of bytes_per_rank bytes per rank - one untimed of each, which opens RCCL's
// channels, then kMeasureReps timed ones whose MEDIAN counts (a single sample at 64 MB sits within the run-to-run spread of the
// threshold it decides) - HIP events on the context stream around the stream-ordered forms, wall time around the blocking ones.  The
// rate of a collective is what a rank RECEIVED from the others divided by the time and by the world - 1 links it arrived over (xGMI
// is point-to-point: GB/s per link and direction, the unit of SP_OPT_LINK_GBS); the minimum over the ranks is stored, so that every
// rank draws the same conclusion from it.  bytes_per_rank = 0 only reads the stored figures back.
//
// Every rank issues the SAME sequence of collectives whatever fails locally: (1) everything local - payload buffers,
// events - is prepared before the first collective; (2) a 32-byte status word per rank goes round through the slot reserved at
// sp_ctx_create, on every path: one rank that could not prepare makes EVERY rank skip the timed collectives, zero its figures and
// return the same error; (3) inside the timed part a local HIP error (an event that cannot be recorded or read) costs the figure, not
// the collective - the call is still made - and (4) the closing word carries status and rates: a failure anywhere zeroes the figures
// everywhere, so that mode 2 of SP_OPT_SHARD_INTERPOLATION can never pick different collective sequences on different ranks.  Only a
// transport that itself reports failure ends the sequence early: its communicator is in an unknown state and nothing sent through it
// could be trusted (callers bound that case with their own deadline, as they do for sp_comm_selftest).
namespace {
constexpr int kMeasureReps = 3;
// all-gather of one 32-byte word per rank through the reserved slot; all[4 r .. 4 r + 3] = rank r's word
int agree_words(sp_ctx* c, const double mine[4], std::vector<double>& all) {
    const uint64_t W = (uint64_t)c->world;
    all.assign(4 * W, 0.0);
    uint8_t* slot = static_cast<uint8_t*>(c->d_agree);
    if (hipMemcpy(slot, mine, 32, hipMemcpyHostToDevice) != hipSuccess) {      // (the peers are owed the collective all the same)
        (void)hipGetLastError();
        (void)hipMemset(slot, 0xff, 32);                                       // an all-ones word reads as NaN: "this rank failed"
    }
    if (c->allgather(c->allgather_user, slot, slot + 32, 32) != 0) { sp_set_error("sp_comm_measure: the transport failed"); return SP_E_HIP; }
    if (hipMemcpy(all.data(), slot + 32, W * 32, hipMemcpyDeviceToHost) != hipSuccess) { sp_set_error("sp_comm_measure: reading the agreement words back failed"); return SP_E_HIP; }
    return SP_OK;
}
}  // namespace

int sp_comm_measure(sp_ctx* c, uint64_t bytes_per_rank, double out[6]) {
    if (!c || bytes_per_rank % 8) return SP_E_INVALID_ARG;
    if (bytes_per_rank == 0 || c->world < 2) {
        if (out) for (int i = 0; i < 6; ++i) out[i] = c->measured_link[i];
        return SP_OK;
    }
    if (!c->allgather) { sp_set_error("sp_comm_measure: no collective installed"); return SP_E_STATE; }
    if ((uint64_t)c->world > sp_ctx::kAgreeMaxWorld) { sp_set_error("sp_comm_measure: world too large"); return SP_E_INVALID_ARG; }
    const uint64_t W = (uint64_t)c->world, per_pair = std::max<uint64_t>(8, (bytes_per_rank / W) & ~(uint64_t)7);
    auto forget = [&]() {
        for (double& x : c->measured_link) x = 0.0;
        delete c->prover_state_deleter_holder;      // (a shape set up under the old figure is set up again)
        c->prover_state_deleter_holder = nullptr;
    };
    // (1) local preparation, no collective yet
    DevBuf send, recv;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto prepare = [&]() -> int {
        SP_HIP_CHECK(hipSetDevice(c->device));
        SP_TRY(send.alloc(std::max(bytes_per_rank, W * per_pair)));
        SP_TRY(recv.alloc(std::max(W * bytes_per_rank, W * per_pair)));
        SP_HIP_CHECK(hipMemsetAsync(send.p, 0x5a, std::max(bytes_per_rank, W * per_pair), c->stream));
        SP_HIP_CHECK(hipStreamSynchronize(c->stream));
        SP_HIP_CHECK(hipEventCreate(&e0));
        SP_HIP_CHECK(hipEventCreate(&e1));
        return SP_OK;
    };
    int local = prepare();
    if (const char* f = std::getenv("SP_COMM_MEASURE_FAULT_RANK")) if (std::atoi(f) == c->rank) local = SP_E_ALLOC;   // (the tests' fault injection)
    struct Events { hipEvent_t &a, &b; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } events_guard{e0, e1};
    // (2) is every rank ready?
    std::vector<double> all;
    const double ready[4] = {local == SP_OK ? 1.0 : 0.0, 0.0, 0.0, 0.0};
    int rc = agree_words(c, ready, all);
    if (rc != SP_OK) { forget(); return rc; }
    for (uint64_t r = 0; r < W; ++r)
        // (a zero word is also what the timing-only transport delivers for the ranks that do not exist: only a rank that SAYS it failed counts -
        //  its own word is never zero there)
        if (!(all[4 * r] == 1.0) && !(all[4 * r] == 0.0 && r != (uint64_t)c->rank && c->comm_is_null)) {
            forget();
            if (local != SP_OK) return local;
            sp_set_error("sp_comm_measure: rank " + std::to_string(r) + " could not prepare its buffers; nothing was measured on any rank");
            return SP_E_STATE;
        }
    // (3) the timed collectives: the same calls on every rank; a local timing error costs the figure only
    bool figures_ok = true, transport_ok = true;
    auto timed = [&](bool a2a, double* median_ms) {
        double ms[kMeasureReps] = {};
        for (int rep = 0; rep <= kMeasureReps && transport_ok; ++rep) {      // rep 0 opens the channels
            const auto t0 = std::chrono::steady_clock::now();
            int trc = 0;
            double took = 0.0;
            if (a2a ? (c->alltoall_async != nullptr) : (c->allgather_async != nullptr)) {
                bool ev = hipEventRecord(e0, c->stream) == hipSuccess;
                trc = a2a ? c->alltoall_async(c->allgather_user, send.p, recv.p, per_pair, c->stream) : c->allgather_async(c->allgather_user, send.p, recv.p, bytes_per_rank, c->stream);
                ev = (hipEventRecord(e1, c->stream) == hipSuccess) && ev;
                ev = (hipStreamSynchronize(c->stream) == hipSuccess) && ev;
                float f = 0.f;
                ev = ev && hipEventElapsedTime(&f, e0, e1) == hipSuccess;
                if (!ev) { (void)hipGetLastError(); figures_ok = false; }
                took = (double)f;
            } else {
                trc = a2a ? c->alltoall(c->allgather_user, send.p, recv.p, per_pair) : c->allgather(c->allgather_user, send.p, recv.p, bytes_per_rank);
                took = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
            if (trc != 0) transport_ok = false;
            if (rep > 0) ms[rep - 1] = took;
        }
        std::sort(ms, ms + kMeasureReps);
        *median_ms = ms[kMeasureReps / 2];
    };
    double ag_ms = 0.0, a2a_ms = 0.0;
    timed(false, &ag_ms);
    if (transport_ok && (c->alltoall || c->alltoall_async)) timed(true, &a2a_ms);
    if (!transport_ok) { forget(); sp_set_error("sp_comm_measure: the transport failed"); return SP_E_HIP; }
    // (4) status and rates of every rank; the minimum over the ranks
    const double mine[4] = {figures_ok ? 1.0 : 0.0,
                            ag_ms > 0 ? (double)bytes_per_rank / (ag_ms * 1e-3) / 1e9 : 0.0,        // (W - 1) B received over W - 1 links
                            a2a_ms > 0 ? (double)per_pair / (a2a_ms * 1e-3) / 1e9 : 0.0, 0.0};
    rc = agree_words(c, mine, all);
    if (rc != SP_OK) { forget(); return rc; }
    double ag_min = mine[1], a2a_min = mine[2];
    for (uint64_t r = 0; r < W; ++r) {
        if (all[4 * r] == 0.0 && r != (uint64_t)c->rank && c->comm_is_null) continue;     // a rank that does not exist (timing-only transport)
        if (!(all[4 * r] == 1.0)) {
            forget();
            sp_set_error("sp_comm_measure: rank " + std::to_string(r) + " could not time its collectives; the figures are dropped on every rank");
            return SP_E_STATE;
        }
        if (all[4 * r + 1] > 0) ag_min = std::min(ag_min, all[4 * r + 1]);
        if (all[4 * r + 2] > 0) a2a_min = std::min(a2a_min, all[4 * r + 2]);
    }
    c->measured_link[0] = ag_ms; c->measured_link[1] = ag_min; c->measured_link[2] = a2a_ms; c->measured_link[3] = a2a_min;
    c->measured_link[4] = (double)bytes_per_rank; c->measured_link[5] = (double)W;
    if (out) for (int i = 0; i < 6; ++i) out[i] = c->measured_link[i];
    // (the prover reads the figure in setup(): a shape set up under the old one is set up again)
    delete c->prover_state_deleter_holder;
    c->prover_state_deleter_holder = nullptr;
    return SP_OK;
}

// Exercises the installed transport: every rank contributes rank-stamped blocks to an all-gather and (when an all-to-all hook
// exists) to an all-to-all, and checks what comes back.  0 = both primitives deliver the documented layout.
int sp_comm_selftest(sp_ctx* c, uint64_t bytes_per_block) {
    if (!c || bytes_per_block == 0 || bytes_per_block % 8) return SP_E_INVALID_ARG;
    if (c->world > 1 && !c->allgather) { sp_set_error("sp_comm_selftest: no collective installed"); return SP_E_STATE; }
    SP_HIP_CHECK(hipSetDevice(c->device));
    const uint64_t W = (uint64_t)c->world, words = bytes_per_block / 8;
    DevBuf send, recv;
    SP_TRY(send.alloc(W * bytes_per_block));
    SP_TRY(recv.alloc(W * bytes_per_block));
    std::vector<uint64_t> h(W * words), back(W * words);
    auto stamp = [&](uint64_t from, uint64_t to, uint64_t k) { return (from << 48) ^ (to << 32) ^ (k * 0x9e3779b97f4a7c15ull); };
    // all-gather: this rank's block, recv[s] = block of rank s
    for (uint64_t k = 0; k < words; ++k) h[k] = stamp((uint64_t)c->rank, 0xffff, k);
    SP_HIP_CHECK(hipMemcpy(send.p, h.data(), bytes_per_block, hipMemcpyHostToDevice));
    SP_HIP_CHECK(hipMemset(recv.p, 0, W * bytes_per_block));
    if (c->allgather) {
        if (c->allgather(c->allgather_user, send.p, recv.p, bytes_per_block) != 0) { sp_set_error("sp_comm_selftest: all-gather hook failed"); return SP_E_HIP; }
    } else {
        SP_HIP_CHECK(hipMemcpy(recv.p, send.p, bytes_per_block, hipMemcpyDeviceToDevice));
    }
    SP_HIP_CHECK(hipMemcpy(back.data(), recv.p, W * bytes_per_block, hipMemcpyDeviceToHost));
    for (uint64_t s2 = 0; s2 < W; ++s2)
        for (uint64_t k = 0; k < words; ++k)
            if (back[s2 * words + k] != stamp(s2, 0xffff, k)) { sp_set_error("sp_comm_selftest: all-gather delivered a wrong block"); return SP_E_HIP; }
    // all-to-all: block d goes to rank d, recv[s] = the block rank s addressed to this rank
    if (c->alltoall) {
        for (uint64_t d = 0; d < W; ++d)
            for (uint64_t k = 0; k < words; ++k) h[d * words + k] = stamp((uint64_t)c->rank, d, k);
        SP_HIP_CHECK(hipMemcpy(send.p, h.data(), W * bytes_per_block, hipMemcpyHostToDevice));
        SP_HIP_CHECK(hipMemset(recv.p, 0, W * bytes_per_block));
        if (c->alltoall(c->allgather_user, send.p, recv.p, bytes_per_block) != 0) { sp_set_error("sp_comm_selftest: all-to-all hook failed"); return SP_E_HIP; }
        SP_HIP_CHECK(hipMemcpy(back.data(), recv.p, W * bytes_per_block, hipMemcpyDeviceToHost));
        for (uint64_t s2 = 0; s2 < W; ++s2)
            for (uint64_t k = 0; k < words; ++k)
                if (back[s2 * words + k] != stamp(s2, (uint64_t)c->rank, k)) { sp_set_error("sp_comm_selftest: all-to-all delivered a wrong block"); return SP_E_HIP; }
    }
    // the stream-ordered forms, enqueued on the context stream between two copies like the prover enqueues them between kernels
    if (c->allgather_async) {
        for (uint64_t k = 0; k < words; ++k) h[k] = stamp((uint64_t)c->rank, 0xfffe, k);
        SP_HIP_CHECK(hipMemcpyAsync(send.p, h.data(), bytes_per_block, hipMemcpyHostToDevice, c->stream));
        SP_HIP_CHECK(hipMemsetAsync(recv.p, 0, W * bytes_per_block, c->stream));
        if (c->allgather_async(c->allgather_user, send.p, recv.p, bytes_per_block, c->stream) != 0) { sp_set_error("sp_comm_selftest: stream-ordered all-gather failed"); return SP_E_HIP; }
        SP_HIP_CHECK(hipMemcpyAsync(back.data(), recv.p, W * bytes_per_block, hipMemcpyDeviceToHost, c->stream));
        SP_HIP_CHECK(hipStreamSynchronize(c->stream));
        for (uint64_t s2 = 0; s2 < W; ++s2)
            for (uint64_t k = 0; k < words; ++k)
                if (back[s2 * words + k] != stamp(s2, 0xfffe, k)) { sp_set_error("sp_comm_selftest: the stream-ordered all-gather delivered a wrong block"); return SP_E_HIP; }
    }
    if (c->alltoall_async) {
        for (uint64_t d = 0; d < W; ++d)
            for (uint64_t k = 0; k < words; ++k) h[d * words + k] = stamp((uint64_t)c->rank, d + 0x100, k);
        SP_HIP_CHECK(hipMemcpyAsync(send.p, h.data(), W * bytes_per_block, hipMemcpyHostToDevice, c->stream));
        SP_HIP_CHECK(hipMemsetAsync(recv.p, 0, W * bytes_per_block, c->stream));
        if (c->alltoall_async(c->allgather_user, send.p, recv.p, bytes_per_block, c->stream) != 0) { sp_set_error("sp_comm_selftest: stream-ordered all-to-all failed"); return SP_E_HIP; }
        SP_HIP_CHECK(hipMemcpyAsync(back.data(), recv.p, W * bytes_per_block, hipMemcpyDeviceToHost, c->stream));
        SP_HIP_CHECK(hipStreamSynchronize(c->stream));
        for (uint64_t s2 = 0; s2 < W; ++s2)
            for (uint64_t k = 0; k < words; ++k)
                if (back[s2 * words + k] != stamp(s2, (uint64_t)c->rank + 0x100, k)) { sp_set_error("sp_comm_selftest: the stream-ordered all-to-all delivered a wrong block"); return SP_E_HIP; }
    }
    return SP_OK;
}

int sp_sync(sp_ctx* c) {
    if (!c) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    SP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return SP_OK;
}

int sp_last_kernel_ms(sp_ctx* c, float* ms) {
    if (!c || !ms) return SP_E_INVALID_ARG;
    if (c->last_pending) {
        SP_HIP_CHECK(hipEventSynchronize(c->ev1));
        SP_HIP_CHECK(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
        c->last_pending = false;
    }
    *ms = c->last_ms;
    return SP_OK;
}

// upload `count` ABI-encoded elements and decode them into the device layout
static int upload_decode(sp_ctx* c, const uint8_t* host, uint64_t count, fe* dst_dev) {
    DevBuf raw;
    SP_TRY(raw.alloc(count * 32));
    SP_HIP_CHECK(hipMemcpyAsync(raw.p, host, count * 32, hipMemcpyHostToDevice, c->stream));
    SP_TRY(decode_elements(c->stream, c->enc, raw.as<uint8_t>(), count, dst_dev));
    SP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return SP_OK;
}
static int encode_download(sp_ctx* c, const fe* src_dev, uint64_t count, uint8_t* host) {
    DevBuf raw;
    SP_TRY(raw.alloc(count * 32));
    SP_TRY(encode_elements(c->stream, c->enc, src_dev, count, raw.as<uint8_t>()));
    SP_HIP_CHECK(hipMemcpyAsync(host, raw.p, count * 32, hipMemcpyDeviceToHost, c->stream));
    SP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return SP_OK;
}
static int decode_one(sp_ctx* c, const uint8_t* in, fe* out) {
    return sp_fe_to_device(c->enc, in, 1, reinterpret_cast<uint8_t*>(out));
}

static int ntt_dev_impl(sp_ctx* c, fe* data, uint64_t n, uint32_t batch, int inverse, const uint8_t* coset, fe* tmp) {
    int k = sp_log2_exact(n);
    if (k < 0 || k > 30) { sp_set_error("ntt: size must be a power of two <= 2^30"); return SP_E_INVALID_ARG; }
    NttEngine& e = *c->ntt;
    fe h;
    if (coset) SP_TRY(decode_one(c, coset, &h));
    // the engine's natural->natural transforms are out of place: src = data, dst = tmp, then copy back
    if (!inverse) {
        if (coset) SP_TRY(e.scale_by_powers(data, n, batch, n, h, nullptr));
        SP_TRY(e.forward_natural(data, tmp, k, batch, n, n, data));  // result lands back in `data`
        return SP_OK;
    } else {
        SP_TRY(e.inverse_natural(data, tmp, k, batch, n));
        if (coset) {
            if (fe_is_zero(h)) return SP_E_ZERO_INVERSE;
            SP_TRY(e.scale_by_powers(data, n, batch, n, fe_inv(h), nullptr));
        }
    }
    return SP_OK;
}

int sp_ntt(sp_ctx* c, uint8_t* data, uint64_t n, int inverse, const uint8_t* coset) {
    if (!c || !data) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    if (sp_log2_exact(n) < 0) { sp_set_error("ntt: size must be a power of two"); return SP_E_INVALID_ARG; }
    DevBuf a, b;
    SP_TRY(a.alloc(n * sizeof(fe)));
    SP_TRY(b.alloc(n * sizeof(fe)));
    SP_TRY(upload_decode(c, data, n, a.as<fe>()));
    SP_TRY(ntt_dev_impl(c, a.as<fe>(), n, 1, inverse, coset, b.as<fe>()));
    SP_TRY(encode_download(c, a.as<fe>(), n, data));
    return SP_OK;
}

int sp_ntt_dev(sp_ctx* c, void* data_dev, uint64_t n, uint32_t batch, int inverse, const uint8_t* coset) {
    if (!c || !data_dev || batch == 0) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    int k = sp_log2_exact(n);
    if (k < 0) return SP_E_INVALID_ARG;
    size_t need = sizeof(fe) * n * batch;
    if (c->scratch_bytes < need) {
        if (c->scratch) (void)hipFree(c->scratch);
        c->scratch = nullptr; c->scratch_bytes = 0;
        if (hipMalloc(&c->scratch, need) != hipSuccess) { sp_set_error("hipMalloc scratch failed"); return SP_E_ALLOC; }
        c->scratch_bytes = need;
    }
    // make sure twiddle tables exist before the timed region
    const fe* t = nullptr;
    SP_TRY(c->ntt->roots(k, &t));
    SP_HIP_CHECK(hipEventRecord(c->ev0, c->stream));
    int rc = ntt_dev_impl(c, reinterpret_cast<fe*>(data_dev), n, batch, inverse, coset, reinterpret_cast<fe*>(c->scratch));
    SP_HIP_CHECK(hipEventRecord(c->ev1, c->stream));
    if (rc != SP_OK) return rc;
    c->last_pending = true;  // resolved by sp_last_kernel_ms (the call itself stays asynchronous)
    return SP_OK;
}

// HIP-event timer on the context stream around an arbitrary sequence of asynchronous calls (bench.py's timed region).
int sp_timer_start(sp_ctx* c) {
    if (!c) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    SP_HIP_CHECK(hipEventRecord(c->tev0, c->stream));
    return SP_OK;
}
int sp_timer_stop(sp_ctx* c, float* ms) {
    if (!c || !ms) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    SP_HIP_CHECK(hipEventRecord(c->tev1, c->stream));
    SP_HIP_CHECK(hipEventSynchronize(c->tev1));
    SP_HIP_CHECK(hipEventElapsedTime(ms, c->tev0, c->tev1));
    return SP_OK;
}

int sp_lde(sp_ctx* c, const uint8_t* coeffs, uint64_t n, uint32_t cols, uint32_t blowup, const uint8_t* coset, uint8_t* out) {
    if (!c || !coeffs || !coset || !out || cols == 0) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    int k = sp_log2_exact(n), lb = sp_log2_exact(blowup);
    if (k < 0 || lb < 0 || k + lb > 30) { sp_set_error("lde: n and blowup must be powers of two"); return SP_E_INVALID_ARG; }
    uint64_t N = n << lb;
    fe h;
    SP_TRY(decode_one(c, coset, &h));
    DevBuf a, b, d;
    SP_TRY(a.alloc(n * cols * sizeof(fe)));
    SP_TRY(b.alloc(n * cols * sizeof(fe)));
    SP_TRY(d.alloc(N * cols * sizeof(fe)));
    SP_TRY(upload_decode(c, coeffs, n * cols, a.as<fe>()));
    NttEngine& e = *c->ntt;
    // natural coefficients -> h-scaled, bit-reversed: forward_natural's gather pass wants natural input, so go through
    // evaluations: a (coefficients) --scale h^k--> --forward NTT (natural)--> evaluations on h<g>; then the engine's
    // iNTT leaves them as bit-reversed h-scaled coefficients x n, fixed by the 1/n post scalar folded in scale_by_powers.
    // Simpler and exact: bit-reverse by running DIF inverse on the forward transform.
    SP_TRY(e.scale_by_powers(a.as<fe>(), n, cols, n, h, nullptr));
    SP_TRY(e.forward_natural(a.as<fe>(), b.as<fe>(), k, cols, n, n));                // evaluations over <g> of p(h x)
    SP_TRY(e.dif_natural_to_bitrev_inverse(b.as<fe>(), k, cols, n, nullptr));       // n * (c_j h^j), bit-reversed
    fe ninv = fe_inv(fe_from_u64(n));
    SP_TRY(e.scale_by_powers(b.as<fe>(), n, cols, n, fe_one(), &ninv));
    SP_TRY(e.lde_from_bitrev(b.as<fe>(), d.as<fe>(), k, lb, cols, n, N));
    SP_TRY(encode_download(c, d.as<fe>(), N * cols, out));
    return SP_OK;
}

// ---- the transform drivers as the prover calls them (sp_lde_dev, sp_intt_bitrev_dev) and their pass lists (sp_ntt_plan) ----
namespace {
// [p, p + ((vectors - 1) * stride + len) * 32): the bytes `vectors` arrays of `len` elements at `stride` elements span
bool extents_overlap(const void* a, uint64_t a_elems, const void* b, uint64_t b_elems) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_elems * sizeof(fe) && b0 < a0 + a_elems * sizeof(fe);
}
// *out = (vectors - 1) * stride + len, the elements `vectors` arrays of `len` at `stride` span; false when that does not fit 2^48
// elements (2^53 bytes: no device holds it, and nothing computed from it below can wrap)
bool span_elems(uint64_t vectors, uint64_t stride, uint64_t len, uint64_t* out) {
    uint64_t prod = 0;
    if (vectors == 0 || __builtin_mul_overflow(vectors - 1, stride, &prod) || __builtin_add_overflow(prod, len, out)) return false;
    return *out < (1ull << 48);
}
// vectors x 2^logL elements in one launch: the launcher refuses 2^31 work-groups and a tile may be a single element
bool launch_fits(uint64_t vectors, int logL) { return vectors >= 1 && vectors < (1ull << 31) && (vectors << logL) < (1ull << 31); }
static_assert((int)NTT_DRV_FORWARD_NATURAL == SP_NTT_DRIVER_FORWARD_NATURAL && (int)NTT_DRV_INVERSE_NATURAL == SP_NTT_DRIVER_INVERSE_NATURAL &&
              (int)NTT_DRV_DIT_BITREV_TO_NATURAL == SP_NTT_DRIVER_DIT_BITREV_TO_NATURAL && (int)NTT_DRV_DIF_NATURAL_TO_BITREV_INVERSE == SP_NTT_DRIVER_INTT_BITREV &&
              (int)NTT_DRV_LDE_FROM_BITREV == SP_NTT_DRIVER_LDE_NATURAL && (int)NTT_DRV_LDE_COSET_MAJOR == SP_NTT_DRIVER_LDE_COSET_MAJOR,
              "sp_ntt_plan hands the header's driver numbers to ntt_plan");
static_assert(NTT_LOAD_GATHER_BITREV == 1 && NTT_LOAD_EXPAND == 2 && NTT_STORE_SCATTER_BITREV == 1, "sp_ntt_pass documents these numbers");
}  // namespace

int sp_lde_dev(sp_ctx* c, const void* coeffs_dev, void* out_dev, uint64_t n, uint32_t blowup, uint32_t cols, uint64_t src_stride,
               uint64_t dst_stride, int order, uint32_t shard_log, uint32_t shard_rank) {
    if (!c || !coeffs_dev || !out_dev || cols == 0) return SP_E_INVALID_ARG;
    if (order != SP_LDE_NATURAL && order != SP_LDE_COSET_MAJOR) { sp_set_error("sp_lde_dev: unknown order"); return SP_E_INVALID_ARG; }
    const int k = sp_log2_exact(n), lb = sp_log2_exact(blowup);
    if (k < 0 || lb < 0 || k + lb > 30) { sp_set_error("sp_lde_dev: n and blowup must be powers of two, n * blowup <= 2^30"); return SP_E_INVALID_ARG; }
    if (shard_log > (uint32_t)lb || shard_rank >= (1u << shard_log)) { sp_set_error("sp_lde_dev: shard_log <= log2(blowup) and shard_rank < 2^shard_log"); return SP_E_INVALID_ARG; }
    const uint64_t b_loc = (uint64_t)blowup >> shard_log, out_len = n * b_loc;
    if (src_stride < n || dst_stride < out_len) { sp_set_error("sp_lde_dev: src_stride >= n and dst_stride >= n * (blowup >> shard_log)"); return SP_E_INVALID_ARG; }
    uint64_t src_span = 0, dst_span = 0;
    if (!launch_fits((uint64_t)cols * b_loc, k) || !span_elems(cols, src_stride, n, &src_span) || !span_elems(cols, dst_stride, out_len, &dst_span)) { sp_set_error("sp_lde_dev: too many columns for one launch, or strides beyond any allocation"); return SP_E_INVALID_ARG; }
    if (extents_overlap(coeffs_dev, src_span, out_dev, dst_span)) { sp_set_error("sp_lde_dev: coefficients and output overlap"); return SP_E_INVALID_ARG; }
    SP_HIP_CHECK(hipSetDevice(c->device));
    const fe* src = reinterpret_cast<const fe*>(coeffs_dev);
    fe* dst = reinterpret_cast<fe*>(out_dev);
    if (order == SP_LDE_COSET_MAJOR) return c->ntt->lde_coset_major(src, dst, k, lb, cols, src_stride, dst_stride, (int)shard_log, (int)shard_rank);
    return c->ntt->lde_from_bitrev(src, dst, k, lb, cols, src_stride, dst_stride, (int)shard_log, (int)shard_rank);
}

int sp_intt_bitrev_dev(sp_ctx* c, void* data_dev, uint64_t n, uint32_t batch, uint64_t stride, const void* post_table_dev, const void* src_dev) {
    if (!c || !data_dev || batch == 0) return SP_E_INVALID_ARG;
    const int k = sp_log2_exact(n);
    if (k < 0 || k > 30) { sp_set_error("sp_intt_bitrev_dev: n must be a power of two <= 2^30"); return SP_E_INVALID_ARG; }
    if (stride < n) { sp_set_error("sp_intt_bitrev_dev: stride >= n"); return SP_E_INVALID_ARG; }
    uint64_t span = 0;
    if (!launch_fits(batch, k) || !span_elems(batch, stride, n, &span)) { sp_set_error("sp_intt_bitrev_dev: too many vectors for one launch, or a stride beyond any allocation"); return SP_E_INVALID_ARG; }
    if (src_dev && extents_overlap(src_dev, span, data_dev, span)) { sp_set_error("sp_intt_bitrev_dev: src overlaps data (pass NULL to transform in place)"); return SP_E_INVALID_ARG; }
    if (post_table_dev && extents_overlap(post_table_dev, n, data_dev, span)) { sp_set_error("sp_intt_bitrev_dev: post_table overlaps data"); return SP_E_INVALID_ARG; }
    SP_HIP_CHECK(hipSetDevice(c->device));
    return c->ntt->dif_natural_to_bitrev_inverse(reinterpret_cast<fe*>(data_dev), k, batch, stride, reinterpret_cast<const fe*>(post_table_dev),
                                                 reinterpret_cast<const fe*>(src_dev));
}

int sp_ntt_plan(int driver, uint32_t k, uint32_t logb, uint32_t shard_log, uint32_t batch, sp_ntt_pass* out, uint32_t cap, uint32_t* count_out) {
    if (!count_out || batch == 0 || driver < SP_NTT_DRIVER_FORWARD_NATURAL || driver > SP_NTT_DRIVER_LDE_COSET_MAJOR) return SP_E_INVALID_ARG;
    const bool lde = driver == SP_NTT_DRIVER_LDE_NATURAL || driver == SP_NTT_DRIVER_LDE_COSET_MAJOR;
    if (k > 30 || logb > 30 || k + logb > 30 || shard_log > logb || (!lde && logb != 0)) { sp_set_error("sp_ntt_plan: k + logb <= 30, shard_log <= logb, logb = 0 unless the driver is an LDE"); return SP_E_INVALID_ARG; }
    if (!launch_fits((uint64_t)batch << (logb - shard_log), (int)k)) { sp_set_error("sp_ntt_plan: too many vectors for one launch"); return SP_E_INVALID_ARG; }
    const std::vector<NttPlannedPass> plan = ntt_plan((NttDriver)driver, (int)k, (int)logb, (int)shard_log, batch);
    *count_out = (uint32_t)plan.size();
    if (!out) return SP_OK;
    if (cap < plan.size()) { sp_set_error("sp_ntt_plan: the driver launches more passes than cap"); return SP_E_INVALID_ARG; }
    for (size_t i = 0; i < plan.size(); ++i) {
        const NttPlannedPass& p = plan[i];
        out[i] = sp_ntt_pass{p.dif ? 1u : 0u, (uint32_t)p.load, (uint32_t)p.store, p.contig ? 1u : 0u, p.gtw ? 1u : 0u, p.s, p.r, p.g,
                             p.radix4, p.xcd_map, p.weak_out, p.stage_tw, p.logL, p.tiles, p.vectors, p.coset_count};
    }
    return SP_OK;
}

// The periodic-column table of the prover (prover.cpp air_periodic_tables: the routine composition_air calls), for one column,
// handed back in natural order: out[j b + c] = table entry (c, j).  Canonical big-endian whatever the context's encoding.
int sp_air_periodic_lde(sp_ctx* c, const sp_air_periodic_column* col, uint64_t n, uint32_t blowup, const uint8_t coset[32], uint8_t* out) {
    if (!c || !col || !coset || !out) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    const int k = sp_log2_exact(n), lb = sp_log2_exact(blowup), lp = col->period ? sp_log2_exact(col->period) : -1;
    if (k < 0 || lb < 1 || k + lb > 30 || lp < 0 || lp > k || !col->values) {
        sp_set_error("sp_air_periodic_lde: n, blowup (>= 2) and the period must be powers of two, 1 <= period <= n");
        return SP_E_INVALID_ARG;
    }
    const uint64_t p = col->period, M = p << lb;
    std::vector<fe> hv(p), ht(M);
    for (uint64_t j = 0; j < p; ++j) hv[j] = fe_from_bytes_be(col->values + 32 * j);
    DevBuf vals, ws, tab;
    SP_TRY(vals.alloc(p * sizeof(fe)));
    SP_TRY(ws.alloc(p * sizeof(fe)));
    SP_TRY(tab.alloc(M * sizeof(fe)));
    SP_HIP_CHECK(hipMemcpyAsync(vals.p, hv.data(), p * sizeof(fe), hipMemcpyHostToDevice, c->stream));
    SP_TRY(air_periodic_tables(c->stream, *c->ntt, vals.as<fe>(), ws.as<fe>(), tab.as<fe>(), 1, (uint32_t)lp, (uint32_t)k, (uint32_t)lb, fe_from_bytes_be(coset)));
    SP_HIP_CHECK(hipMemcpyAsync(ht.data(), tab.p, M * sizeof(fe), hipMemcpyDeviceToHost, c->stream));
    SP_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (uint64_t cc = 0; cc < blowup; ++cc)
        for (uint64_t j = 0; j < p; ++j) fe_to_bytes_be(ht[cc * p + j], out + 32 * (j * blowup + cc));
    return SP_OK;
}

// One stride class's 1 / Z table as composition_air builds it (air_stride_tables + batch_inverse), handed back in natural order:
// out[j b + c] = table entry (c, j).  Canonical big-endian whatever the context's encoding.
int sp_air_stride_table(sp_ctx* c, uint32_t period, uint32_t offset, uint64_t n, uint32_t blowup, const uint8_t coset[32], uint8_t* out) {
    if (!c || !coset || !out) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    const int k = sp_log2_exact(n), lb = sp_log2_exact(blowup), ls = period ? sp_log2_exact(period) : -1;
    if (k < 0 || lb < 1 || k + lb > 30 || ls < 0 || ls > k || offset >= period) {
        sp_set_error("sp_air_stride_table: n, blowup (>= 2) and the period must be powers of two, 1 <= period <= n, offset < period");
        return SP_E_INVALID_ARG;
    }
    const uint64_t M = (uint64_t)period << lb;
    DevBuf tab;   // [M] U, [M] U - g^(o n/s) -> 1 / Z, [M] scratch
    SP_TRY(tab.alloc(3 * M * sizeof(fe)));
    fe* u = tab.as<fe>();
    SP_HIP_CHECK(hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
    SP_TRY(air_stride_class_tables(c->stream, *c->ntt, u, u + M, (uint32_t)ls, offset, (uint32_t)k, (uint32_t)lb, fe_from_bytes_be(coset)));
    SP_TRY(batch_inverse(c->stream, u + M, u + 2 * M, M, c->d_flag));
    std::vector<fe> ht(M);
    int flag = 0;
    SP_HIP_CHECK(hipMemcpyAsync(ht.data(), u + M, M * sizeof(fe), hipMemcpyDeviceToHost, c->stream));
    SP_HIP_CHECK(hipMemcpyAsync(&flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SP_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (flag) { sp_set_error("sp_air_stride_table: the zerofier vanishes on the coset"); return SP_E_ZERO_INVERSE; }
    for (uint64_t cc = 0; cc < blowup; ++cc)
        for (uint64_t j = 0; j < period; ++j) fe_to_bytes_be(ht[cc * period + j], out + 32 * (j * blowup + cc));
    return SP_OK;
}

static sp::MerkleHash ctx_merkle_hash(const sp_ctx* c, uint32_t fe_per_leaf) {
    if (c->opt_merkle_backend != SP_MERKLE_POSEIDON) return sp::MerkleHash::KECCAK256;
    // one element per leaf: the single-element tree of a FRI layer (hash_single) unless the caller asked for the row tree the prover
    // commits a one-column trace segment with (hash_many over one element): SP_OPT_MERKLE_ONE_COLUMN_ROWS
    return (fe_per_leaf == 1 && !c->opt_merkle_one_column_rows) ? sp::MerkleHash::POSEIDON_SINGLE : sp::MerkleHash::POSEIDON_BATCH;
}
int sp_merkle_build(sp_ctx* c, const uint8_t* leaves, uint64_t n_leaves, uint32_t fe_per_leaf, uint8_t root_out[32], uint8_t* nodes_out) {
    if (!c || !leaves || !root_out || fe_per_leaf == 0) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    if (sp_log2_exact(n_leaves) < 0) { sp_set_error("merkle: leaf count must be a power of two"); return SP_E_INVALID_ARG; }
    DevBuf raw, cols, nodes;
    uint64_t total = n_leaves * fe_per_leaf;
    SP_TRY(raw.alloc(total * 32));
    SP_TRY(cols.alloc(total * sizeof(fe)));
    SP_TRY(nodes.alloc((2 * n_leaves - 1) * sizeof(digest32)));
    SP_HIP_CHECK(hipMemcpyAsync(raw.p, leaves, total * 32, hipMemcpyHostToDevice, c->stream));
    SP_TRY(rows_to_columns(c->stream, c->enc, raw.as<uint8_t>(), n_leaves, fe_per_leaf, cols.as<fe>(), n_leaves));
    const MerkleHash mh = ctx_merkle_hash(c, fe_per_leaf);
    SP_TRY(merkle_hash_leaves(c->stream, cols.as<fe>(), n_leaves, fe_per_leaf, n_leaves, nodes.as<digest32>(), LdeOrder{0, 0, 0}, mh));
    SP_TRY(merkle_reduce(c->stream, nodes.as<digest32>(), n_leaves, nullptr, mh));
    SP_HIP_CHECK(hipMemcpyAsync(root_out, nodes.p, 32, hipMemcpyDeviceToHost, c->stream));
    if (nodes_out) SP_HIP_CHECK(hipMemcpyAsync(nodes_out, nodes.p, (2 * n_leaves - 1) * 32, hipMemcpyDeviceToHost, c->stream));
    SP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return SP_OK;
}

int sp_merkle_build_dev(sp_ctx* c, const void* cols_dev, uint64_t n_leaves, uint32_t fe_per_leaf, uint64_t col_stride, void* nodes_dev) {
    if (!c || !cols_dev || !nodes_dev || fe_per_leaf == 0 || col_stride < n_leaves) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    if (sp_log2_exact(n_leaves) < 0) { sp_set_error("merkle: leaf count must be a power of two"); return SP_E_INVALID_ARG; }
    SP_HIP_CHECK(hipEventRecord(c->ev0, c->stream));
    const MerkleHash mh = ctx_merkle_hash(c, fe_per_leaf);
    int rc = merkle_hash_leaves(c->stream, reinterpret_cast<const fe*>(cols_dev), col_stride, fe_per_leaf, n_leaves, reinterpret_cast<digest32*>(nodes_dev), LdeOrder{0, 0, 0}, mh);
    if (rc == SP_OK) rc = merkle_reduce(c->stream, reinterpret_cast<digest32*>(nodes_dev), n_leaves, nullptr, mh);
    SP_HIP_CHECK(hipEventRecord(c->ev1, c->stream));
    if (rc != SP_OK) return rc;
    c->last_pending = true;
    return SP_OK;
}

int sp_batch_inverse(sp_ctx* c, uint8_t* data, uint64_t n) {
    if (!c || !data) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    if (n == 0) return SP_OK;
    DevBuf a, s;
    SP_TRY(a.alloc(n * sizeof(fe)));
    SP_TRY(s.alloc(n * sizeof(fe)));
    SP_TRY(upload_decode(c, data, n, a.as<fe>()));
    SP_HIP_CHECK(hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
    SP_TRY(batch_inverse(c->stream, a.as<fe>(), s.as<fe>(), n, c->d_flag));
    int flag = 0;
    SP_HIP_CHECK(hipMemcpyAsync(&flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SP_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (flag) { sp_set_error("batch inverse of a zero element"); return SP_E_ZERO_INVERSE; }
    SP_TRY(encode_download(c, a.as<fe>(), n, data));
    return SP_OK;
}

int sp_fe_mul(sp_ctx* c, const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out) {
    if (!c || !a || !out) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c->device));
    if (n == 0) return SP_OK;
    DevBuf x, y, r;
    SP_TRY(x.alloc(n * sizeof(fe)));
    SP_TRY(r.alloc(n * sizeof(fe)));
    SP_TRY(upload_decode(c, a, n, x.as<fe>()));
    if (b) {
        SP_TRY(y.alloc(n * sizeof(fe)));
        SP_TRY(upload_decode(c, b, n, y.as<fe>()));
    }
    SP_TRY(mul_elements(c->stream, x.as<fe>(), b ? y.as<fe>() : nullptr, n, r.as<fe>()));
    SP_TRY(encode_download(c, r.as<fe>(), n, out));
    return SP_OK;
}

}  // extern "C"
