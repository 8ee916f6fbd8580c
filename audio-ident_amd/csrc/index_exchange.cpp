// index_exchange.cpp -- the hash index between ranks: aid_comm (an RCCL communicator) and the exchange of index
// shards, in steps a host-driven exchange runs around its own collectives (shard_info, reserve, pack, splice) or in
// one call over RCCL (aid_index_allgather). The only file of libaidfp.so that includes RCCL; the index itself is
// index_host.cpp.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstring>

#include "engine_internal.h"

struct aid_comm {
    ncclComm_t comm = nullptr;
    int world = 0, rank = 0, device = -1;
};

#define NCCL_TRY(expr)                                                                              \
    do {                                                                                            \
        ncclResult_t r_ = (expr);                                                                   \
        if (r_ != ncclSuccess) return fail(AID_ERR_DEVICE, std::string(#expr ": ") + ncclGetErrorString(r_)); \
    } while (0)

extern "C" {

int aid_comm_id(uint8_t id[AID_COMM_ID_BYTES]) {
    if (!id) return fail(AID_ERR_INVALID, "null id");
    ncclUniqueId u;
    NCCL_TRY(ncclGetUniqueId(&u));
    static_assert(sizeof(u.internal) == AID_COMM_ID_BYTES, "RCCL unique id size");
    std::memcpy(id, u.internal, AID_COMM_ID_BYTES);
    return AID_OK;
}

int aid_comm_create(aid_engine *e, const uint8_t id[AID_COMM_ID_BYTES], int32_t world, int32_t rank, aid_comm **out) {
    if (!e || !id || !out || world <= 0 || rank < 0 || rank >= world) return fail(AID_ERR_INVALID, "aid_comm_create: bad argument");
    *out = nullptr;
    {
        EngineCall call(e);
        if (call.rc) return call.rc;
        HIP_TRY(e->idx.g_meta.reserve(2 * (size_t)world + 2));  // the exchange's (count, n_tracks) and ok rounds
    }
    ncclUniqueId u;
    std::memcpy(u.internal, id, AID_COMM_ID_BYTES);
    ncclComm_t c = nullptr;
    NCCL_TRY(ncclCommInitRank(&c, world, u, rank));
    aid_comm *ac = new aid_comm();
    ac->comm = c;
    ac->world = world;
    ac->rank = rank;
    ac->device = e->device;
    *out = ac;
    return AID_OK;
}

void aid_comm_destroy(aid_comm *c) {
    if (!c) return;
    if (c->comm) {
        (void)hipSetDevice(c->device);
        (void)ncclCommDestroy(c->comm);
    }
    delete c;
}

int aid_comm_size(const aid_comm *c, int32_t *world, int32_t *rank) {
    if (!c || !c->comm) return fail(AID_ERR_INVALID, "aid_comm_size: null comm");
    int n = 0, r = 0;
    NCCL_TRY(ncclCommCount(c->comm, &n));
    NCCL_TRY(ncclCommUserRank(c->comm, &r));
    if (world) *world = n;
    if (rank) *rank = r;
    return AID_OK;
}

// the exchange in three steps (aid_index_allgather runs them around two RCCL all-gathers; a host-driven
// exchange, e.g. torch.distributed over gloo, runs them around its own collectives). Engine lock held and the
// append settled (the entry point's EngineCall), all of them
static int shard_info_locked(aid_engine *e, int64_t first, int64_t *count, uint32_t *n_tracks) {
    if (first < 0 || first > e->idx.n_post) return fail(AID_ERR_INVALID, "index exchange: first out of range");
    *count = e->idx.n_post - first;
    *n_tracks = e->idx.n_tracks;
    return AID_OK;
}

static int pack_locked(aid_engine *e, int64_t first, uint32_t *planes, int64_t stride, hipStream_t s) {
    if (e->idx.inject_exchange_fail) {  // test hook: this rank's prepare step fails as a device OOM would
        e->idx.inject_exchange_fail = 0;
        return fail(AID_ERR_NOMEM, "index exchange: injected failure of this rank's pack (aid_engine_force)");
    }
    const int64_t n = e->idx.n_post - first;
    if (n > stride) return fail(AID_ERR_INVALID, "aid_index_pack: stride below the shard's count");
    const uint32_t *src[3] = {e->idx.p_hash.p, e->idx.p_track.p, e->idx.p_t.p};
    for (int q = 0; q < 3 && n > 0; ++q)
        HIP_TRY(hipMemcpyAsync(planes + q * stride, src[q] + first, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    if (stride > n)  // padding: defined bytes on the wire
        for (int q = 0; q < 3; ++q)
            HIP_TRY(hipMemsetAsync(planes + q * stride + n, 0, (stride - n) * sizeof(uint32_t), s));
    return AID_OK;
}

// everything a splice of `tot` postings at `first` (and n_tracks ids) can fail on, done before the exchange:
// the posting planes and the tombstone buffer grow keeping every stored posting (n_post, not first) and
// every tombstone; the index itself (n_post, n_tracks, the CSR) does not change
static int splice_reserve_locked(aid_engine *e, int64_t first, int64_t tot, uint32_t n_tracks, hipStream_t s) {
    if (first < 0 || first > e->idx.n_post) return fail(AID_ERR_INVALID, "index exchange: first out of range");
    if (tot < 0) return fail(AID_ERR_INVALID, "index exchange: negative posting count");
    if (first + tot > 0xFFFFFFFFll) return fail(AID_ERR_INVALID, "index exchange: more than 2^32 postings");
    const size_t want = (size_t)std::max<int64_t>(first + tot, e->idx.n_post);
    if (int rc = grow_postings(e, want, s)) return rc;
    return n_tracks > e->idx.n_tracks ? reserve_tracks(e, n_tracks, s) : AID_OK;
}

// failure-atomic: everything that can fail (growth of the posting planes and track tables) happens before
// the index changes; the union then replaces [first, n_post) in one stream-ordered pass
static int splice_locked(aid_engine *e, int64_t first, const uint32_t *recv, int32_t world, int64_t stride,
                         const int64_t *counts, uint32_t n_tracks, hipStream_t s) {
    if (first < 0 || first > e->idx.n_post) return fail(AID_ERR_INVALID, "aid_index_splice: first out of range");
    int64_t tot = 0;
    for (int r = 0; r < world; ++r) {
        if (counts[r] < 0 || counts[r] > stride) return fail(AID_ERR_INVALID, "aid_index_splice: bad count");
        tot += counts[r];
    }
    if (int rc = splice_reserve_locked(e, first, tot, n_tracks, s)) return rc;
    if (int rc = ensure_tracks(e, n_tracks, s)) return rc;  // capacity reserved: only the commit is left
    uint32_t *dst[3] = {e->idx.p_hash.p, e->idx.p_track.p, e->idx.p_t.p};
    int64_t at = first;
    for (int r = 0; r < world; ++r) {
        const int64_t n = counts[r];
        for (int q = 0; q < 3 && n > 0; ++q)
            HIP_TRY(hipMemcpyAsync(dst[q] + at, recv + ((size_t)r * 3 + q) * stride, n * sizeof(uint32_t),
                                   hipMemcpyDeviceToDevice, s));
        at += n;
    }
    HIP_TRY(hipStreamSynchronize(s));
    e->idx.n_post = at;
    e->idx.drop_main(kFallSplice);
    return AID_OK;
}

int aid_index_shard_info(aid_engine *e, int64_t first, int64_t *count, uint32_t *n_tracks) {
    if (!e || !count || !n_tracks) return fail(AID_ERR_INVALID, "aid_index_shard_info: null argument");
    EngineCall call(e, nullptr, true);
    return call.rc ? call.rc : shard_info_locked(e, first, count, n_tracks);
}

int aid_index_reserve(aid_engine *e, int64_t first, int64_t total, uint32_t n_tracks, void *stream) {
    if (!e) return fail(AID_ERR_INVALID, "aid_index_reserve: null engine");
    EngineCall call(e, stream, true, kOrderLast);
    return call.rc ? call.rc : splice_reserve_locked(e, first, total, n_tracks, call.s);
}

int aid_index_pack(aid_engine *e, int64_t first, uint32_t *planes, int64_t stride, void *stream) {
    if (!e || (!planes && stride > 0) || stride < 0) return fail(AID_ERR_INVALID, "aid_index_pack: bad argument");
    EngineCall call(e, stream, true);
    if (call.rc) return call.rc;
    if (first < 0 || first > e->idx.n_post) return fail(AID_ERR_INVALID, "aid_index_pack: first out of range");
    if (int rc = EngineCall::wait_last(e, call.s, kOrderLast)) return rc;
    if (int rc = pack_locked(e, first, planes, stride, call.s)) return rc;
    HIP_TRY(hipStreamSynchronize(call.s));
    return AID_OK;
}

int aid_index_splice(aid_engine *e, int64_t first, const uint32_t *recv, int32_t world, int64_t stride,
                     const int64_t *counts, uint32_t n_tracks, void *stream) {
    if (!e || world <= 0 || stride < 0 || !counts || (!recv && stride > 0))
        return fail(AID_ERR_INVALID, "aid_index_splice: bad argument");
    EngineCall call(e, stream, true, kOrderLast);
    return call.rc ? call.rc : splice_locked(e, first, recv, world, stride, counts, n_tracks, call.s);
}

// one all-gather of an int64 pair per rank over the engine's meta buffer (reserved by aid_comm_create);
// every rank calls it the same number of times, whatever its own state
static int allgather_pair(aid_engine *e, aid_comm *c, int64_t a, int64_t b, std::vector<int64_t> &out, hipStream_t s) {
    const int W = c->world;
    const int64_t mine[2] = {a, b};
    HIP_TRY(hipMemcpyAsync(e->idx.g_meta.p, mine, sizeof(mine), hipMemcpyHostToDevice, s));
    NCCL_TRY(ncclAllGather(e->idx.g_meta.p, e->idx.g_meta.p + 2, 2, ncclInt64, c->comm, s));
    out.assign(2 * (size_t)W, 0);
    HIP_TRY(hipMemcpyAsync(out.data(), e->idx.g_meta.p + 2, out.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return AID_OK;
}

int aid_index_allgather(aid_engine *e, aid_comm *c, int64_t first, int64_t *n_total) {
    if (!e || !c || !c->comm) return fail(AID_ERR_INVALID, "aid_index_allgather: null argument");
    if (c->device != e->device) return fail(AID_ERR_INVALID, "aid_index_allgather: comm and engine on different devices");
    EngineCall call(e, nullptr, true, kDrainLast);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    const int W = c->world;
    // aid_comm_create reserved this engine's meta buffer; a comm made with another engine gets it here (16 B per
    // rank: returning early instead would leave the other ranks blocked in the first all-gather)
    HIP_TRY(e->idx.g_meta.reserve(2 * (size_t)W + 2));
    // Every rank runs the same collectives whatever happens locally: (1) (count, n_tracks), (2) one ok flag
    // per rank after every step that can fail locally, (3) the payload only when every rank is ready. A
    // rank-local failure (bad arguments, OOM of the exchange buffers or the grown index, the pack) is
    // therefore seen by all ranks before the payload all-gather, and every rank returns an error with its
    // index unchanged instead of leaving its peers blocked in RCCL.
    int64_t n_local = -1;
    uint32_t nt = 0;
    const int bad = shard_info_locked(e, first, &n_local, &nt);
    std::vector<int64_t> meta;
    if (int rc = allgather_pair(e, c, bad ? -1 : n_local, (int64_t)nt, meta, s)) return rc;
    int64_t mx = 0, tot = 0;
    uint32_t tracks = 0;
    std::vector<int64_t> counts(W);
    for (int r = 0; r < W; ++r) {
        if (meta[2 * r] < 0) return bad ? bad : fail(AID_ERR_INVALID, "aid_index_allgather: another rank's shard is invalid");
        counts[r] = meta[2 * r];
        mx = std::max(mx, counts[r]);
        tot += counts[r];
        tracks = std::max(tracks, (uint32_t)meta[2 * r + 1]);
    }
    // 2. local preparation: the exchange buffers ([3][mx] own planes, [W][3][mx] received; scratch of this
    //    call only: ~(W + 1) x 12 B per largest-shard posting), the grown index, the pack of the own shard
    int rc = AID_OK;
    if (mx > 0) {
        hipError_t he = e->idx.g_send.reserve(3 * (size_t)mx);
        if (he == hipSuccess) he = e->idx.g_recv.reserve(3 * (size_t)mx * W);
        if (he != hipSuccess)
            rc = fail(he == hipErrorOutOfMemory ? AID_ERR_NOMEM : AID_ERR_DEVICE,
                      std::string("index exchange buffers: ") + hipGetErrorString(he));
        if (!rc) rc = splice_reserve_locked(e, first, tot, tracks, s);
        if (!rc) rc = pack_locked(e, first, e->idx.g_send.p, mx, s);
        if (!rc) {
            he = hipStreamSynchronize(s);
            if (he != hipSuccess) rc = fail(AID_ERR_DEVICE, std::string("index exchange pack: ") + hipGetErrorString(he));
        }
    } else {
        rc = splice_reserve_locked(e, first, 0, tracks, s);
    }
    const std::string local_err = rc ? last_error_text() : std::string();
    std::vector<int64_t> ok;
    if (int rc2 = allgather_pair(e, c, rc ? 0 : 1, (int64_t)rc, ok, s)) {
        e->idx.g_send.release();
        e->idx.g_recv.release();
        return rc2;
    }
    int failed = -1;
    for (int r = 0; r < W && failed < 0; ++r)
        if (!ok[2 * r]) failed = r;
    if (failed >= 0) {
        e->idx.g_send.release();
        e->idx.g_recv.release();
        if (rc) return fail(rc, local_err);
        return fail(AID_ERR_STATE, "index exchange aborted: rank " + std::to_string(failed) +
                                       " failed to prepare (error " + std::to_string(ok[2 * failed + 1]) +
                                       "); this rank's index is unchanged");
    }
    if (mx > 0) {
        // 3. one all-gather of the padded planes, then the union in rank order replaces this rank's shard
        NCCL_TRY(ncclAllGather(e->idx.g_send.p, e->idx.g_recv.p, 3 * (size_t)mx, ncclUint32, c->comm, s));
        rc = splice_locked(e, first, e->idx.g_recv.p, W, mx, counts.data(), tracks, s);
        e->idx.g_send.release();
        e->idx.g_recv.release();
        if (rc) return rc;
    } else if (int rc3 = ensure_tracks(e, tracks, s)) {
        return rc3;
    }
    if (n_total) *n_total = e->idx.n_post;
    return AID_OK;
}

}  // extern "C"
