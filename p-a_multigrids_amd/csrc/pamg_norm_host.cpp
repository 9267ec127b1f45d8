// The reductions of libpamg on the host side (pamg_norm.hip's launches): one pass over a
// level, the ranks' records combined, and the checks of the norm entry points.
#include <algorithm>
#include <cmath>

#include "pamg_host.h"

using namespace pamg;
using namespace pamg::host;

namespace {

// ---- convergence control (pamg_norm.hip) ---------------------------------------
// A reduction of level l on the handle's stream: a state field, or (field == nullptr) the residual
// A tnew - RHS computed in registers and not stored. Device scratch: the rank's record, the gathered
// records (one per rank), the slab of per-workgroup partials. One hipMemcpyAsync into the pinned host
// buffer and one bounded stream wait; on a partition the ranks' records are combined in rank order.
NormRec norm_identity() { return NormRec{-HUGE_VAL, 0.0, 0.0, 0ull}; }

NormRec norm_join(const NormRec &a, const NormRec &b) {
    return NormRec{std::fmax(a.max, b.max), std::fmax(a.maxabs, b.maxabs), a.sumsq + b.sumsq,
                   a.nonfinite | b.nonfinite};
}

}  // namespace

namespace pamg {
namespace host {

double norm_value(const NormRec &r, int kind) {
    if (r.nonfinite) return std::nan("");
    switch (kind) {
        case PAMG_NORM_REF: return r.max > 0.0 ? r.max : 0.0;   // get_convergence's loop starts from 0.0 (:879)
        case PAMG_NORM_MAXABS: return r.maxabs;
        case PAMG_NORM_L1: return r.sumsq;   // the pass accumulated |v| into the sum word (norm_mode)
        default: return std::sqrt(r.sumsq);  // L2: the squares; L2_MASS: v^T M v per sub-element
    }
}

// the kinds of the residual forms (pamg_residual_norm, pamg_get_convergence, pamg_solve)
bool norm_kind_ok(int kind) { return kind == PAMG_NORM_REF || kind == PAMG_NORM_MAXABS || kind == PAMG_NORM_L2; }

// ... and of pamg_field_norm / pamg_error_norm
bool field_kind_ok(int kind) { return norm_kind_ok(kind) || kind == PAMG_NORM_L1 || kind == PAMG_NORM_L2_MASS; }

// what a reduction pass accumulates into the record's sum word for `kind` (pamg_norm_device.h kAcc*)
int norm_mode(int kind) { return kind == PAMG_NORM_L1 ? 1 : kind == PAMG_NORM_L2_MASS ? 2 : 0; }

int norm_reduce(pamg_handle *h, int l, const double *field, int form, int mode, NormRec *res) {
    Level &L = h->lv[l];
    const bool residual_form = form == kFormResidual;
    const bool face = residual_form && h->p.op == 1;
    if (h->comm && !h->comm->nccl && !h->comm->local) {
        h->err = "norm: the communicator was aborted";
        return PAMG_ERR_COMM;
    }
    const bool rccl = h->comm && h->comm->nccl, local = h->comm && h->comm->local;
    const int ng = rccl || local ? h->nranks : 1;   // records combined (a detached partition: its own)
    const size_t nslab = face ? face_norm_slab_records(L) : norm_slab_records(L);
    CHK(ensure_scratch(h, (1 + (size_t)ng + nslab) * sizeof(NormRec)));
    if (face) CHK(monitor_setup(h));
    if (!h->norm_host)
        HIPCHK(h, hipHostMalloc((void **)&h->norm_host, ((size_t)std::max(h->nranks, 1) + 1) * sizeof(NormRec),
                                hipHostMallocDefault));
    NormRec *d_rec = reinterpret_cast<NormRec *>(h->scratch), *d_all = d_rec + 1, *d_slab = d_all + ng;
    NormRec *host = h->norm_host;
    const bool empty = L.N == 0;   // a rank that owns nothing: no launch, the identities
    if (face) {
        // tnew and RHS in, the operator (168 B), face (8 kFaceStride) and selector (16 B) records, the words read
        // and written (24 B each way per boundary position), the exchanged words (24 B out, 24 B in); an empty
        // rank launches nothing but still meets its peers in the exchange (it has none) and in the gather
        const HaloPlan &P = L.halo;
        Span sp(h, PAMG_K_NORM, 48.0 * (double)L.N + (168.0 + 8.0 * kFaceStride + 16.0) * h->U +
                                    48.0 * (double)h->U * P.nbpos + 24.0 * (double)(P.remote.size() + P.recv_dst.size()));
        HIPCHK(h, launch_face_monitor_words(h->stream, L, h->U, h->mon_img, h->mon_send));
        CHK(monitor_exchange(h, l));
        HIPCHK(h, launch_face_residual_reduce(h->stream, L, h->mon_img, l == 1, 1 / h->p.dt, h->slots, d_slab, d_rec));
    } else if (!empty) {
        Span sp(h, PAMG_K_NORM, residual_form ? 48.0 * (double)L.N + 168.0 * h->U : 24.0 * (double)L.N);
        if (residual_form) HIPCHK(h, launch_residual_reduce(h->stream, L, 1 / h->p.dt, d_slab, d_rec));
        else if (form == kFormError) HIPCHK(h, launch_error_reduce(h->stream, L, h->geo1, mode, d_slab, d_rec));
        else HIPCHK(h, launch_field_reduce(h->stream, L, field, mode, d_slab, d_rec));
    }
    if (rccl) {
        if (empty) {
            host[ng] = norm_identity();
            HIPCHK(h, hipMemcpyAsync(d_rec, &host[ng], sizeof(NormRec), hipMemcpyHostToDevice, h->stream));
        }
        // one all-gather of the records (4 words each), settled and aborted on failure as a halo exchange is
        const ncclResult_t r = ncclAllGather(d_rec, d_all, sizeof(NormRec) / sizeof(uint64_t), ncclUint64,
                                             h->comm->nccl, h->stream);
        const int rc = nccl_settle(h->comm->nccl, r, local_timeout_s(), h->err, "ncclAllGather (norm)");
        if (rc != PAMG_OK) {
            (void)ncclCommAbort(h->comm->nccl);
            h->comm->nccl = nullptr;
            return rc;
        }
        HIPCHK(h, hipMemcpyAsync(host, d_all, (size_t)ng * sizeof(NormRec), hipMemcpyDeviceToHost, h->stream));
        CHK(sync_stream(h, h->stream));
        CHK(comm_error(h));
    } else {
        NormRec mine = norm_identity();
        if (!empty) {
            HIPCHK(h, hipMemcpyAsync(host, d_rec, sizeof(NormRec), hipMemcpyDeviceToHost, h->stream));
            CHK(sync_stream(h, h->stream));
            mine = host[0];
        }
        if (local) CHK(norm_meet_local(h, mine, host));
        else host[0] = mine;
    }
    NormRec out = host[0];
    for (int r = 1; r < ng; ++r) out = norm_join(out, host[r]);
    *res = out;
    return PAMG_OK;
}

// the agglomerated coarsest level of an op = 1 partition is replicated on every rank, not partitioned
int norm_level_ok(pamg_handle *h, int level) {
    if (h->agg && level == h->p.multi_levels) {
        h->err = "norm: the agglomerated coarsest level of an op = 1 partition is replicated, not partitioned";
        return PAMG_ERR_ARG;
    }
    return PAMG_OK;
}

int residual_norm_ok(pamg_handle *h) {
    if (h->p.op == 1 && h->p.monitor != 1) {
        h->err = "residual norm: op = 1's residual first rewrites the halo words, so it cannot be read-only "
                 "(use pamg_get_convergence, or create the handle with monitor = 1)";
        return PAMG_ERR_ARG;
    }
    if (h->p.solver == 2) {
        h->err = "residual norm: solver 2's level-1 residual re-assembles the RHS, so it cannot be read-only "
                 "(use pamg_get_convergence)";
        return PAMG_ERR_ARG;
    }
    if (h->p.op == 1 && h->nranks > 1 && !h->comm) {
        h->err = "residual norm: a detached partition (no transport bound) cannot see its peers' tnew, which "
                 "op = 1's residual reads across the un_ele faces";
        return PAMG_ERR_STATE;
    }
    return PAMG_OK;
}

int residual_norm(pamg_handle *h, int level, int kind, double *value) {
    NormRec r;
    CHK(norm_reduce(h, level, nullptr, kFormResidual, 0, &r));
    *value = norm_value(r, kind);
    return PAMG_OK;
}

// tracer(1)%error: its three planes on the first call that names the field, zero-filled (the reference's
// allocation, :239) -- as monitor_setup does for the monitor's image, so a run that never asks for the field
// keeps its footprint. A failed allocation leaves the handle as it was
int error_setup(pamg_handle *h) {
    Level &L = h->lv[1];
    if (L.ERR) return PAMG_OK;
    double *e = nullptr;
    CHK(dev_alloc(h, &e, 3 * (size_t)L.pitch));
    if (hipMemsetAsync(e, 0, 3 * (size_t)L.pitch * sizeof(double), h->stream) != hipSuccess) {
        (void)hipGetLastError();
        dev_free(e);
        h->err = "error field: hipMemsetAsync failed";
        return PAMG_ERR_HIP;
    }
    L.ERR = e;
    return PAMG_OK;
}

}  // namespace host
}  // namespace pamg
