// The host layer of libpamg, shared by its translation units (not part of the C-ABI): the transports'
// records, the error-return macros, the timing span, the device-memory helpers and one declaration of
// every host function that is called across files. The files, each one subsystem:
//   pamg_comm.cpp       the transports (RCCL, the in-process local group), the halo exchange, timing, scratch
//   pamg_face_host.cpp  op = 1: the smoother call (chain, gates), the two-sweep passes, the agglomerated
//                       coarsest level, the fused and corrected face cycles, the convergence monitor
//   pamg_cycle.cpp      the per-step operations and the op = 0 cycle drivers with their call schedules
//   pamg_norm_host.cpp  the reductions
//   pamg_api.cpp        the C entry points
// The per-step smoother (pamg_cycle.cpp smooth) and the face call (pamg_face_host.cpp face_call) use each
// other's subsystem, and every host wait first drains the chain gates (face_gates_drain); otherwise a file
// calls only the ones listed before it.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

#include "pamg_internal.h"

namespace pamg {
// Single-process device-copy transport (pamg_comm_local_group): n partition handles of one
// owner map, each driven by its own host thread like one process per rank. The exchange is
// the RCCL one with ncclSend / ncclRecv replaced by device-to-device copies between the
// handles: a rank posts its packed send words (pointer + an event recorded after the
// packing) to every peer, pulls each peer's words for it into its own receive buffer behind
// that peer's event, and then waits, before it may repack, until every peer has issued its
// reads of its words (the send completion of ncclSend). Posts carry a per-pair sequence
// number, so ranks meet exchange by exchange as grouped send/recv calls do.
struct LocalGroup {
    struct Post { long seq = 0; const double *ptr = nullptr; hipEvent_t ev = nullptr; int64_t pitch = 0; };
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Post> ready, done;   // [src * n + dst]
    // the ranks' reduction records of a norm (norm_meet_local): a slot per rank with the sequence number of
    // the reduction it belongs to, two sets used alternately (a rank posts reduction q + 2 only after every
    // rank has posted q + 1, that is after every rank has read q's slots)
    struct NormSlot { long seq = 0; NormRec rec{}; };
    std::vector<NormSlot> norm;      // [(seq & 1) * n + rank]
    int refs = 0;
};
struct Comm {
    ncclComm_t nccl = nullptr;
    LocalGroup *local = nullptr;
    std::vector<long> seq;           // per peer index (level 1's plan): exchanges completed
    long norm_seq = 0;               // reductions this rank has taken to the local group
    hipEvent_t ev_ready = nullptr, ev_done = nullptr;
};
}  // namespace pamg

#define HIPCHK(h, expr)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                 \
            return PAMG_ERR_HIP;                                                          \
        }                                                                                 \
    } while (0)

#define NCCLCHK(h, expr)                                                                  \
    do {                                                                                  \
        ncclResult_t r_ = (expr);                                                         \
        if (r_ != ncclSuccess) {                                                          \
            (h)->err = std::string(#expr) + ": " + ncclGetErrorString(r_);                \
            return PAMG_ERR_COMM;                                                         \
        }                                                                                 \
    } while (0)

#define CHK(expr)                    \
    do {                             \
        int rc_ = (expr);            \
        if (rc_ != PAMG_OK) return rc_; \
    } while (0)

// ncclSend / ncclRecv inside a group only enqueue (a non-blocking communicator may answer ncclInProgress)
#define NCCLQ(h, expr)                                                                    \
    do {                                                                                  \
        ncclResult_t r_ = (expr);                                                         \
        if (r_ != ncclSuccess && r_ != ncclInProgress) {                                  \
            (void)ncclGroupEnd();                                                         \
            (h)->err = std::string(#expr) + ": " + ncclGetErrorString(r_);                \
            return PAMG_ERR_COMM;                                                         \
        }                                                                                 \
    } while (0)

// PAMG_RHS_TOLD_HALO (A/B builds): k_rhs writes the compact told copy of the halo at the start of a
// step (1) or k_told_halo gathers it afterwards (0, default: the folded form measured 1.4 % slower
// on the time loop, scripts/ab_tl.sh, profiles/r01_v17_time_loop.txt)
#ifndef PAMG_RHS_TOLD_HALO
#define PAMG_RHS_TOLD_HALO 0
#endif

namespace pamg {
// the host functions shared between the files: hidden, so the library's dynamic symbol table holds the C-ABI only
namespace host __attribute__((visibility("hidden"))) {

// ---- pamg_comm.cpp ----
hipEvent_t take_event(pamg_handle *h);
int drain_timing(pamg_handle *h);
int ensure_scratch(pamg_handle *h, size_t bytes);
int local_timeout_s();
int nccl_settle(ncclComm_t c, ncclResult_t r, int limit_s, std::string &err, const char *what);
int nccl_group_end(pamg_handle *h);
int exchange_local(pamg_handle *h, int l, const double *send, hipStream_t st, int w, double *recv);
int exchange(pamg_handle *h, int l, int buf, hipStream_t st, double *dst = nullptr);
int exchange_ring(pamg_handle *h, int c, hipStream_t st);
int xc_setup(pamg_handle *h, int cycles);
int xe_setup(pamg_handle *h);
int halo(pamg_handle *h, int l, double *dst = nullptr);
int halo_async(pamg_handle *h, int buf);
int join_comm(pamg_handle *h);
int settle(pamg_handle *h);
int comm_error(pamg_handle *h);
int sync_stream(pamg_handle *h, hipStream_t s);
void nccl_release(ncclComm_t c);
int norm_meet_local(pamg_handle *h, const NormRec &mine, NormRec *all);

// ---- pamg_face_host.cpp ----
int face_chain_check(pamg_handle *h);
bool face_tiles_ok(pamg_handle *h, int l);
int face_gates_drain(pamg_handle *h);
int face_call(pamg_handle *h, int l, bool src_is_T, int sweeps, bool dead_last, bool res = false, bool both = false);
int face_residual(pamg_handle *h, int l, bool neg);
bool face_cycle_fusable(pamg_handle *h);
int agg_coarse_corrected(pamg_handle *h);
int vcycle_face_fused(pamg_handle *h, int n);
bool face_corrected_pp_ok(pamg_handle *h);
int vcycle_corrected_face_pp(pamg_handle *h, int n);
int agg_create(pamg_handle *h, int U, const double *X, const int *region, const int *neig, const int *fneig,
               const int *dir);
int monitor_setup(pamg_handle *h);
int monitor_exchange(pamg_handle *h, int l);

// ---- pamg_cycle.cpp ----
int smooth(pamg_handle *h, int l, bool src_is_T, int sweeps);
int refresh_told_halo(pamg_handle *h, int l);
int residual(pamg_handle *h, int l);
int restrict_(pamg_handle *h, int l);
int prolong(pamg_handle *h, int l, bool fused_copy);
double vcycle_flops(pamg_handle *h);
int direct_solve(pamg_handle *h, int l);
int smooth_to_tnew(pamg_handle *h, int l, int sweeps);
int residual_corrected(pamg_handle *h, int l);
int call_schedule(pamg_handle *h);
bool fused_ok(pamg_handle *h);
int vcycle_fused(pamg_handle *h, int n, bool dead_after, int steps = 1);
int begin_timestep(pamg_handle *h, bool tnn_dead, bool told_lazy = false, bool defer_rhs = false);
int vcycle(pamg_handle *h, int n, bool dead_after);

// ---- pamg_norm_host.cpp ----
// form: kFormField a state field, kFormResidual A tnew - RHS in registers, kFormError level 1's
// |tnew - sin(x + y)| in registers (get_error's values, not stored); mode: norm_mode(kind).
// kFormResidual with op = 1: the face form -- the monitor words of the level, their exchange, then the
// reduction of the face operator's residual from the monitor's image
enum { kFormField = 0, kFormResidual = 1, kFormError = 2 };
int norm_reduce(pamg_handle *h, int l, const double *field, int form, int mode, NormRec *res);
double norm_value(const NormRec &r, int kind);
bool norm_kind_ok(int kind);
bool field_kind_ok(int kind);
int norm_mode(int kind);
int norm_level_ok(pamg_handle *h, int level);
int residual_norm_ok(pamg_handle *h);
int residual_norm(pamg_handle *h, int level, int kind, double *value);
int error_setup(pamg_handle *h);

template <class T>
int dev_alloc(pamg_handle *h, T **p, size_t count) {
    *p = nullptr;
    if (count == 0) return PAMG_OK;
    HIPCHK(h, hipMalloc((void **)p, count * sizeof(T)));
    return PAMG_OK;
}

// every setup transfer runs on the handle's stream: its streams are non-blocking, so work on
// them is not ordered against the null stream a blocking hipMemcpy uses (a memset queued on
// h->stream could land after such a copy)
// (a host wait on the handle's stream first reads its chain gates back)
template <class T>
int dev_upload(pamg_handle *h, T **p, const std::vector<T> &v) {
    CHK(dev_alloc(h, p, v.size()));
    if (!v.empty()) {
        CHK(face_gates_drain(h));
        HIPCHK(h, hipMemcpyAsync(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));   // v may be freed on return
    }
    return PAMG_OK;
}

inline void dev_free(void *p) {
    if (p) (void)hipFree(p);
}

inline int check_level(pamg_handle *h, int l) {
    if (!h->mesh_ready) { h->err = "mesh not uploaded"; return PAMG_ERR_STATE; }
    if (l < 1 || l > h->p.multi_levels) { h->err = "level out of range"; return PAMG_ERR_ARG; }
    return PAMG_OK;
}

inline double *field_ptr(pamg_handle *h, int l, int what) {
    Level &L = h->lv[l];
    switch (what) {
        case PAMG_TNEW: return L.T;
        case PAMG_TOLD: return L.TOLD;
        case PAMG_RHS: return L.RHS;
        case PAMG_RESIDUAL: return L.RES;
        case PAMG_TNEW_NONLIN: return L.TNN;
        case PAMG_SOURCE: return L.SRC;   // level 1 only (null elsewhere)
        case PAMG_ERROR: return L.ERR;    // level 1 only, and null until error_setup
    }
    return nullptr;
}

// an event pair around the work issued in a scope, on stream s, when its timing class is enabled (one in
// `stride` of its spans). (Events recorded in the resident launch's own dispatch packet, hipExtLaunchKernel,
// measured no cheaper than the marker pair: profiles/r05_a_shape_probe.txt, r05_c_events_ab.txt; removed.)
struct Span {
    pamg_handle *h; int kid; double bytes; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    Span(pamg_handle *h_, int kid_, double bytes_, hipStream_t s_ = nullptr)
        : h(h_->tparent ? h_->tparent : h_), kid(kid_), bytes(bytes_), s(s_ ? s_ : h_->stream) {
        if ((h->timing.mask & (1u << kid)) && h->timing.seq[kid]++ % h->timing.stride == 0) {
            a = take_event(h);
            (void)hipEventRecord(a, s);
        }
    }
    ~Span() {
        if (!a) return;
        b = take_event(h);
        (void)hipEventRecord(b, s);
        h->timing.pending.push_back(Timing::Rec{kid, a, b, bytes});
    }
};

}  // namespace host
}  // namespace pamg
