// The transports of libpamg (RCCL and the in-process local group), the halo exchange with its stream
// bookkeeping, the timing spans' drain, the scratch buffer, and the communicator entry points.
#include <dlfcn.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "pamg_host.h"

using namespace pamg;
using namespace pamg::host;

namespace {

// the communicator (blocking: see nccl_settle); a failure binds nothing to the handle
int nccl_init(pamg_handle *h, ncclComm_t *out, int nranks, ncclUniqueId uid, int rank) {
    *out = nullptr;
    ncclComm_t nc = nullptr;
    const ncclResult_t r = ncclCommInitRank(&nc, nranks, uid, rank);
    if (r != ncclSuccess) {
        h->err = "ncclCommInitRank (rank " + std::to_string(rank) + " of " + std::to_string(nranks) + "): " +
                 ncclGetErrorString(r);
        if (nc) (void)ncclCommAbort(nc);
        return PAMG_ERR_COMM;
    }
    *out = nc;
    return PAMG_OK;
}

}  // namespace

namespace pamg {
namespace host {

// ---- timing -------------------------------------------------------------
hipEvent_t take_event(pamg_handle *h) {
    auto &pool = h->timing.pool;
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

int drain_timing(pamg_handle *h) {
    auto &T = h->timing;
    if (T.pending.empty()) return PAMG_OK;
    // spans may sit on the comm stream (the exchange spans, the early exchange's): the stream joins every
    // exchange in flight first, and the comm stream is drained too, so no event pair is read before it ran
    CHK(settle(h));
    CHK(sync_stream(h, h->stream));
    CHK(sync_stream(h, h->stream_comm));
    for (auto &r : T.pending) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, r.a, r.b));
        T.ms[r.kid] += ms;
        T.count[r.kid] += 1;
        T.bytes[r.kid] += r.bytes;
        T.pool.push_back(r.a);
        T.pool.push_back(r.b);
    }
    T.pending.clear();
    return PAMG_OK;
}

// ---- scratch ------------------------------------------------------------
int ensure_scratch(pamg_handle *h, size_t bytes) {
    if (h->scratch_bytes >= bytes) return PAMG_OK;
    CHK(face_gates_drain(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    dev_free(h->scratch);
    h->scratch = nullptr;
    h->scratch_bytes = 0;
    HIPCHK(h, hipMalloc((void **)&h->scratch, bytes));
    h->scratch_bytes = bytes;
    return PAMG_OK;
}

// ---- halo exchange --------------------------------------------------------
// The halo words of a smoother call are written by the smoother kernel itself
// (local neighbours and boundary values into t_overlap, remote neighbours into
// the packed send buffer); what remains here is the exchange with other ranks.
// pamg_comm_local_group transport: the grouped send/recv below as device copies between the
// partition handles of one process (LocalGroup)
int local_timeout_s() {
    const char *e = getenv("PAMG_COMM_TIMEOUT_S");
    const int t = e ? atoi(e) : 120;
    return t > 0 ? t : 120;
}

// Bounded RCCL waits. A grouped send/recv that answers ncclInProgress is polled here for at
// most PAMG_COMM_TIMEOUT_S (default 120 s, the local group's exchange bound), and every host wait for a stream
// that carries exchanges is bounded the same way (sync_stream); on the bound or an error the communicator is
// aborted, so a rank that stops issuing exchanges ends its peers' calls with PAMG_ERR_COMM instead of hanging
// them. The communicator's initialisation cannot be bounded from here: RCCL 2.27's bootstrap waits for every
// rank, and a non-blocking communicator (ncclConfig_t::blocking = 0) blocked inside ncclCommInitRankConfig
// itself, while a blocking init left on a helper thread faults the process at exit
// (profiles/r06_rccl_init_probe.txt). The caller's launcher bounds it (bench.py: a gloo barrier with a timeout
// right before pamg_comm_init), and the communicator stays blocking.
int nccl_settle(ncclComm_t c, ncclResult_t r, int limit_s, std::string &err, const char *what) {
    const auto t0 = std::chrono::steady_clock::now();
    while (r == ncclInProgress) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(limit_s)) {
            err = std::string(what) + ": not complete within " + std::to_string(limit_s) +
                  " s (PAMG_COMM_TIMEOUT_S); a peer rank did not join or stopped";
            return PAMG_ERR_COMM;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (ncclCommGetAsyncError(c, &r) != ncclSuccess) r = ncclSystemError;
    }
    if (r != ncclSuccess) {
        err = std::string(what) + ": " + ncclGetErrorString(r);
        return PAMG_ERR_COMM;
    }
    return PAMG_OK;
}

// a grouped send/recv's end: polled to completion of its enqueueing; the communicator aborted on failure
int nccl_group_end(pamg_handle *h) {
    const ncclResult_t r = ncclGroupEnd();
    const int rc = nccl_settle(h->comm->nccl, r, local_timeout_s(), h->err, "ncclGroupEnd (halo exchange)");
    if (rc != PAMG_OK) {
        (void)ncclCommAbort(h->comm->nccl);
        h->comm->nccl = nullptr;
    }
    return rc;
}

// w words per entry (6: tnew and told; 3: the tnew words of the resident call's ring), into recv
int exchange_local(pamg_handle *h, int l, const double *send, hipStream_t st, int w, double *recv) {
    Comm &C = *h->comm;
    LocalGroup &G = *C.local;
    const HaloPlan &P = h->lv[l].halo;
    const int me = h->rank, np = (int)P.peers.size();
    std::vector<LocalGroup::Post> got(np);
    auto wait_posts = [&](std::vector<LocalGroup::Post> &box, const char *what) -> int {
        std::unique_lock<std::mutex> lk(G.mu);
        for (int q = 0; q < np; ++q) {
            const int peer = P.peers[q];
            const long want = C.seq[peer] + 1;
            LocalGroup::Post &b = box[(size_t)peer * G.n + me];
            if (!G.cv.wait_for(lk, std::chrono::seconds(local_timeout_s()), [&] { return b.seq >= want; })) {
                h->err = "local halo exchange: rank " + std::to_string(me) + " timed out waiting for rank " +
                         std::to_string(peer) + "'s " + what;
                return PAMG_ERR_COMM;
            }
            if (b.seq != want) { h->err = "local halo exchange: sequence mismatch"; return PAMG_ERR_COMM; }
            got[q] = b;
        }
        return PAMG_OK;
    };
    // 1. post the packed words, pull the peers' words for this rank behind their events
    HIPCHK(h, hipEventRecord(C.ev_ready, st));
    {
        std::lock_guard<std::mutex> lk(G.mu);
        for (int q = 0; q < np; ++q) {
            const int peer = P.peers[q];
            G.ready[(size_t)me * G.n + peer] = {C.seq[peer] + 1, send + w * (size_t)P.send_peer_off[q], C.ev_ready};
        }
    }
    G.cv.notify_all();
    CHK(wait_posts(G.ready, "send words"));
    for (int q = 0; q < np; ++q) {
        const size_t nr = (size_t)(P.recv_peer_off[q + 1] - P.recv_peer_off[q]);
        HIPCHK(h, hipStreamWaitEvent(st, got[q].ev, 0));
        if (nr)
            HIPCHK(h, hipMemcpyAsync(recv + w * (size_t)P.recv_peer_off[q], got[q].ptr, w * nr * sizeof(double),
                                     hipMemcpyDeviceToDevice, st));
    }
    // 2. this rank's reads are issued; its send words may be repacked once every peer's are
    HIPCHK(h, hipEventRecord(C.ev_done, st));
    {
        std::lock_guard<std::mutex> lk(G.mu);
        for (int q = 0; q < np; ++q) {
            const int peer = P.peers[q];
            G.done[(size_t)me * G.n + peer] = {C.seq[peer] + 1, nullptr, C.ev_done};
        }
    }
    G.cv.notify_all();
    CHK(wait_posts(G.done, "receive completion"));
    for (int q = 0; q < np; ++q) {
        HIPCHK(h, hipStreamWaitEvent(st, got[q].ev, 0));
        C.seq[P.peers[q]] += 1;
    }
    return PAMG_OK;
}

// dst: the t_overlap buffer the received words go into (h->tov unless a face call's other snapshot buffer)
int exchange(pamg_handle *h, int l, int buf, hipStream_t st, double *dst) {
    Level &L = h->lv[l];
    const HaloPlan &P = L.halo;
    const double *send = P.send_buf(buf);
    if (!dst) dst = h->tov;
    Span sp(h, PAMG_K_HALO, 2.0 * 48.0 * (double)(P.remote.size() + P.recv_dst.size()), st);
    if (h->comm->local) {
        CHK(exchange_local(h, l, send, st, 6, P.d_recv));
        HIPCHK(h, launch_halo_unpack(st, L, dst, h->tovo));
        return PAMG_OK;
    }
    NCCLCHK(h, ncclGroupStart());
    for (size_t q = 0; q < P.peers.size(); ++q) {
        const int peer = P.peers[q];
        const size_t ns = (size_t)(P.send_peer_off[q + 1] - P.send_peer_off[q]);
        const size_t nr = (size_t)(P.recv_peer_off[q + 1] - P.recv_peer_off[q]);
        if (ns) NCCLQ(h, ncclSend(send + 6 * (size_t)P.send_peer_off[q], 6 * ns, ncclDouble, peer, h->comm->nccl, st));
        if (nr) NCCLQ(h, ncclRecv(P.d_recv + 6 * (size_t)P.recv_peer_off[q], 6 * nr, ncclDouble, peer,
                                  h->comm->nccl, st));
    }
    CHK(nccl_group_end(h));
    HIPCHK(h, launch_halo_unpack(st, L, dst, h->tovo));
    return PAMG_OK;
}

// the tnew words of cycle c of a resident call with halo_exchange = 1 (level 1's ring, 3 words per
// entry; the told words do not change within a time step and travel with the last cycle's exchange)
int exchange_ring(pamg_handle *h, int c, hipStream_t st) {
    Level &L = h->lv[1];
    const HaloPlan &P = L.halo;
    const double *send = P.d_ring + (size_t)c * 3 * P.remote.size();
    Span sp(h, PAMG_K_HALO, 2.0 * 24.0 * (double)(P.remote.size() + P.recv_dst.size()), st);
    if (h->comm->local) {
        CHK(exchange_local(h, 1, send, st, 3, P.d_recv3));
        HIPCHK(h, launch_halo_unpack3(st, L, h->tov));
        return PAMG_OK;
    }
    NCCLCHK(h, ncclGroupStart());
    for (size_t q = 0; q < P.peers.size(); ++q) {
        const int peer = P.peers[q];
        const size_t ns = (size_t)(P.send_peer_off[q + 1] - P.send_peer_off[q]);
        const size_t nr = (size_t)(P.recv_peer_off[q + 1] - P.recv_peer_off[q]);
        if (ns) NCCLQ(h, ncclSend(send + 3 * (size_t)P.send_peer_off[q], 3 * ns, ncclDouble, peer, h->comm->nccl, st));
        if (nr) NCCLQ(h, ncclRecv(P.d_recv3 + 3 * (size_t)P.recv_peer_off[q], 3 * nr, ncclDouble, peer,
                                  h->comm->nccl, st));
    }
    CHK(nccl_group_end(h));
    HIPCHK(h, launch_halo_unpack3(st, L, h->tov));
    return PAMG_OK;
}

// the ring, counters and signal of a resident call of `cycles` cycles with halo_exchange = 1
int xc_setup(pamg_handle *h, int cycles) {
    HaloPlan &P = h->lv[1].halo;
    const int need = cycles - 1;
    if (P.ring_cap < need) {
        CHK(sync_stream(h, h->stream));
        CHK(sync_stream(h, h->stream_comm));
        dev_free(P.d_ring);
        P.d_ring = nullptr;
        P.ring_cap = 0;
        CHK(dev_alloc(h, &P.d_ring, (size_t)need * 3 * P.remote.size()));
        P.ring_cap = need;
    }
    if (!P.d_recv3 && !P.recv_dst.empty()) CHK(dev_alloc(h, &P.d_recv3, 3 * P.recv_dst.size()));
    if (h->xc_cap < need) {
        CHK(sync_stream(h, h->stream));
        dev_free(h->xc_done);
        h->xc_done = nullptr;
        h->xc_cap = 0;
        CHK(dev_alloc(h, &h->xc_done, (size_t)need));
        h->xc_cap = need;
    }
    if (!h->xc_sig) {
        // the comm stream waits on it (hipStreamWaitValue64): HIP's signal memory
        HIPCHK(h, hipExtMallocWithFlags((void **)&h->xc_sig, sizeof(unsigned long long), hipMallocSignalMemory));
        unsigned long long v = 0;
        HIPCHK(h, hipMemcpy(&v, h->xc_sig, sizeof v, hipMemcpyDeviceToHost));
        h->xc_sig_base = v;
    }
    return PAMG_OK;
}

// the early per-call exchange of the resident call: the tile order with the tiles that hold a remote
// face first (they then run in the launch's first round of workgroups, and the exchange of their words
// overlaps the rounds after it), the counter and the signal. PAMG_EARLY_XC=0 turns it off (A/B runs)
int xe_setup(pamg_handle *h) {
    if (h->xe_nremote < 0) {
        std::vector<char> rem;
        vcycle_remote_tiles(h->lv[1], h->U, h->p.n_split, rem);
        std::vector<int> order;
        order.reserve(rem.size());
        for (size_t b = 0; b < rem.size(); ++b)
            if (rem[b]) order.push_back((int)b);
        const int nr = (int)order.size();
        for (size_t b = 0; b < rem.size(); ++b)
            if (!rem[b]) order.push_back((int)b);
        if (nr > 0) CHK(dev_upload(h, &h->xe_map, order));
        h->xe_nremote = nr;
    }
    if (h->xe_nremote > 0 && !h->xe_done) {
        CHK(dev_alloc(h, &h->xe_done, 1));
        HIPCHK(h, hipMemsetAsync(h->xe_done, 0, sizeof(unsigned), h->stream));
        h->xe_total = 0;
    }
    if (h->xe_nremote > 0 && !h->xc_sig) {
        HIPCHK(h, hipExtMallocWithFlags((void **)&h->xc_sig, sizeof(unsigned long long), hipMallocSignalMemory));
        unsigned long long v = 0;
        HIPCHK(h, hipMemcpy(&v, h->xc_sig, sizeof v, hipMemcpyDeviceToHost));
        h->xc_sig_base = v;
    }
    return PAMG_OK;
}

int halo(pamg_handle *h, int l, double *dst) {
    const HaloPlan &P = h->lv[l].halo;
    if (h->comm && !P.peers.empty()) {
        h->lv[l].halo.send_cur = 0;   // the per-step kernels pack into the first buffer
        return exchange(h, l, 0, h->stream, dst);
    }
    return PAMG_OK;
}

// fused V-cycle: the exchange of level 1's words packed into `buf` runs on stream_comm,
// overlapped with the next cycle (nothing in a cycle reads t_overlap)
int halo_async(pamg_handle *h, int buf) {
    HaloPlan &P = h->lv[1].halo;
    P.send_cur = buf;
    if (!h->comm || P.peers.empty()) return PAMG_OK;
    HIPCHK(h, hipEventRecord(h->ev_packed, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream_comm, h->ev_packed, 0));
    CHK(exchange(h, 1, buf, h->stream_comm));
    HIPCHK(h, hipEventRecord(h->ev_sent[buf], h->stream_comm));
    h->sent_pending[buf] = true;
    return PAMG_OK;
}

// `stream` continues after every exchange in flight
int join_comm(pamg_handle *h) {
    for (int b = 0; b < 2; ++b)
        if (h->sent_pending[b]) {
            HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_sent[b], 0));
            h->sent_pending[b] = false;
        }
    return PAMG_OK;
}

// the entry of a call that may read or write what an exchange still in flight touches (the send and receive
// buffers, t_overlap, t_overlap_old): its work waits for the exchange (the resident call's early exchange is
// not joined when the call returns, vcycle_fused). A gated chain launch still unread also blocks the stream
// until the host reads its report (face_gates_drain): every entry reads them first, so no later host wait or
// implicit device synchronisation (hipFree) can wait on a gate that only this thread would open
int settle(pamg_handle *h) {
    CHK(face_gates_drain(h));
    return h->comm ? join_comm(h) : PAMG_OK;
}

// RCCL's asynchronous error state (polled at the ends of the hot-path calls): a
// failed peer or link is reported as PAMG_ERR_COMM instead of a hang in the next exchange
int comm_error(pamg_handle *h) {
    if (!h->comm || !h->comm->nccl) return PAMG_OK;
    ncclResult_t r = ncclSuccess;
    NCCLCHK(h, ncclCommGetAsyncError(h->comm->nccl, &r));
    if (r != ncclSuccess && r != ncclInProgress) {
        h->err = std::string("RCCL asynchronous error: ") + ncclGetErrorString(r);
        (void)ncclCommAbort(h->comm->nccl);
        h->comm->nccl = nullptr;
        return PAMG_ERR_COMM;
    }
    return PAMG_OK;
}

// stream synchronisation that keeps polling RCCL's error state: a rank whose peer failed
// returns PAMG_ERR_COMM (communicator aborted) instead of waiting on a receive that never
// completes; PAMG_COMM_TIMEOUT_S, when set, also bounds the wait. The device-copy transport
// (pamg_comm_local_group) is polled the same way with its exchange bound (PAMG_COMM_TIMEOUT_S,
// default 120 s): its resident call's comm stream waits on a device signal (hipStreamWaitValue64)
// that a faulted or stopped launch would never raise. The poll spins on hipStreamQuery for the first
// PAMG_SYNC_SPIN_MS (default 5 ms; the communicator checked every 256th query), then sleeps 20 us
// between queries and checks the communicator every 16th. A sleep of 20 us lasts ~60 us or more (the
// kernel's timer slack): with the sleeping poll from the start, a rank's 20-cycle call at config 4's
// N = 8 shape (1,024 un_eles, an RCCL self-peer exchange) took 233.7 us against 169.2 us without a
// communicator, its exchange hidden behind the launch (profiles/r05_c_xe_probe.txt)
int sync_stream(pamg_handle *h, hipStream_t s) {
    if (h->tparent) {   // a coarsest-level replica waits as its partition does (the same stream, its exchanges)
        const int rc = sync_stream(h->tparent, s);
        if (rc != PAMG_OK) h->err = h->tparent->err;
        return rc;
    }
    CHK(face_gates_drain(h));
    if (!h->comm || (!h->comm->nccl && !h->comm->local)) {
        HIPCHK(h, hipStreamSynchronize(s));
        return PAMG_OK;
    }
    // PAMG_COMM_TIMEOUT_S (default 120 s) on both transports: a peer that never issues its side of an exchange
    // ends this rank's wait with PAMG_ERR_COMM (RCCL's error state does not report a missing peer)
    const int limit = local_timeout_s();
    constexpr int spin_ms = 5;
    const auto t0 = std::chrono::steady_clock::now();
    const auto spin_end = t0 + std::chrono::milliseconds(spin_ms);
    for (unsigned i = 0;; ++i) {
        const hipError_t e = hipStreamQuery(s);
        if (e == hipSuccess) return PAMG_OK;
        if (e != hipErrorNotReady) HIPCHK(h, e);
        const auto now = std::chrono::steady_clock::now();
        if (now < spin_end && (i & 255) != 255) continue;
        if ((i & 15) == 15 || now < spin_end) CHK(comm_error(h));
        if (limit > 0 && now - t0 > std::chrono::seconds(limit)) {
            if (h->comm->nccl) {
                h->err = "stream did not drain within PAMG_COMM_TIMEOUT_S; RCCL communicator aborted";
                (void)ncclCommAbort(h->comm->nccl);
                h->comm->nccl = nullptr;
            } else {
                h->err = "stream did not drain within PAMG_COMM_TIMEOUT_S (local-group transport)";
            }
            return PAMG_ERR_COMM;
        }
        if (now >= spin_end) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

void nccl_release(ncclComm_t c) { (void)ncclCommDestroy(c); }

// the local group's gather: this rank's record into its slot, every rank's slot of the same reduction out
int norm_meet_local(pamg_handle *h, const NormRec &mine, NormRec *all) {
    Comm &C = *h->comm;
    LocalGroup &G = *C.local;
    const int me = h->rank, n = G.n;
    const long seq = ++C.norm_seq;
    LocalGroup::NormSlot *box = &G.norm[(size_t)(seq & 1) * n];
    std::unique_lock<std::mutex> lk(G.mu);
    box[me].seq = seq;
    box[me].rec = mine;
    G.cv.notify_all();
    for (int r = 0; r < n; ++r) {
        if (!G.cv.wait_for(lk, std::chrono::seconds(local_timeout_s()), [&] { return box[r].seq >= seq; })) {
            h->err = "local norm gather: rank " + std::to_string(me) + " timed out waiting for rank " +
                     std::to_string(r) + "'s record";
            return PAMG_ERR_COMM;
        }
        if (box[r].seq != seq) { h->err = "local norm gather: sequence mismatch"; return PAMG_ERR_COMM; }
        all[r] = box[r].rec;
    }
    return PAMG_OK;
}

}  // namespace host
}  // namespace pamg

extern "C" {

int pamg_comm_unique_id(char out[128]) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return PAMG_ERR_COMM;
    static_assert(sizeof(id) == 128, "ncclUniqueId size");
    std::memcpy(out, &id, 128);
    return PAMG_OK;
}

int pamg_comm_init(pamg_handle *h, int nranks, int rank, const char id[128], int U, const int *owner) {
    if (!h || nranks < 1 || rank < 0 || rank >= nranks || !owner || U < 1) return PAMG_ERR_ARG;
    if (h->mesh_ready) { h->err = "pamg_comm_init must precede pamg_upload_mesh"; return PAMG_ERR_STATE; }
    ncclComm_t nc = nullptr;
    if (nranks > 1 && id) {   // id == NULL: detached partition (pamg_halo_loopback exchanges)
        if (h->comm) { h->err = "communicator already bound"; return PAMG_ERR_STATE; }
        HIPCHK(h, hipSetDevice(h->device));
        ncclUniqueId uid;
        std::memcpy(&uid, id, 128);
        // the communicator, the rank and the owner map are bound to the handle only once RCCL has initialised
        // it (a failure -- a peer that never joins, nccl_init's bound -- leaves the handle as it was, so a retry
        // can bind again)
        CHK(nccl_init(h, &nc, nranks, uid, rank));
    }
    h->nranks = nranks;
    h->rank = rank;
    h->owner.assign(owner, owner + U);
    if (nc) {
        h->comm = new Comm;
        h->comm->nccl = nc;
    }
    return PAMG_OK;
}

int pamg_comm_init_self(pamg_handle *h, const char id[128], int U, const int *part) {
    if (!h || !id || !part || U < 1) return PAMG_ERR_ARG;
    if (h->mesh_ready) { h->err = "pamg_comm_init_self must precede pamg_upload_mesh"; return PAMG_ERR_STATE; }
    if (h->comm) { h->err = "communicator already bound"; return PAMG_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    // the plan and the communicator are bound only once RCCL has initialised it: a failure leaves
    // the handle as it was (no half-bound communicator, no self-peer parts), so a retry can bind
    ncclComm_t nc = nullptr;
    CHK(nccl_init(h, &nc, 1, uid, 0));
    h->nranks = 1;
    h->rank = 0;
    h->owner.assign(U, 0);
    h->vpart.assign(part, part + U);
    h->comm = new Comm;
    h->comm->nccl = nc;
    return PAMG_OK;
}

int pamg_comm_local_group(pamg_handle *const *hs, int n) {
    if (!hs || n < 2) return PAMG_ERR_ARG;
    std::vector<int> seen(n, 0);
    for (int a = 0; a < n; ++a) {
        pamg_handle *h = hs[a];
        if (!h || !h->mesh_ready || h->nranks != n || h->comm || h->rank < 0 || h->rank >= n || seen[h->rank]++)
            return PAMG_ERR_ARG;
        if (h->owner != hs[0]->owner) { h->err = "local group: the partitions' owner maps differ"; return PAMG_ERR_ARG; }
    }
    // create every handle's events first; bind the group only when all of them exist, so a
    // failure leaves no handle half-bound (a retry then sees h->comm == nullptr)
    std::vector<hipEvent_t> evs((size_t)2 * n, nullptr);
    for (int a = 0; a < n; ++a) {
        if (hipSetDevice(hs[a]->device) != hipSuccess ||
            hipEventCreateWithFlags(&evs[2 * a], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&evs[2 * a + 1], hipEventDisableTiming) != hipSuccess) {
            for (hipEvent_t e : evs)
                if (e) (void)hipEventDestroy(e);
            hs[a]->err = "local group: hipEventCreate failed";
            return PAMG_ERR_HIP;
        }
    }
    auto *G = new LocalGroup;
    G->n = n;
    G->ready.resize((size_t)n * n);
    G->done.resize((size_t)n * n);
    G->norm.resize((size_t)2 * n);
    G->refs = n;
    for (int a = 0; a < n; ++a) {
        pamg_handle *h = hs[a];
        h->comm = new Comm;
        h->comm->local = G;
        h->comm->seq.assign(n, 0);
        h->comm->ev_ready = evs[2 * a];
        h->comm->ev_done = evs[2 * a + 1];
    }
    return PAMG_OK;
}

int pamg_comm_info(pamg_handle *h, int *version, char *lib_path, int len) {
    if (!h) return PAMG_ERR_ARG;
    if (version) {
        int v = 0;
        if (ncclGetVersion(&v) != ncclSuccess) return PAMG_ERR_COMM;
        *version = v;
    }
    if (lib_path && len > 0) {
        Dl_info di{};
        const char *p = dladdr((void *)&ncclGetVersion, &di) && di.dli_fname ? di.dli_fname : "";
        std::strncpy(lib_path, p, (size_t)len - 1);
        lib_path[len - 1] = 0;
    }
    return !h->comm ? 0 : h->comm->local ? 2 : 1;
}

}  // extern "C"
