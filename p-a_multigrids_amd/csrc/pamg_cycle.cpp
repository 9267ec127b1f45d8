// The per-step operations of the V-cycle (transport_tri_semi.F90:299-381) and the op = 0 cycle drivers:
// the per-step sequence, the corrected cycle, and the fused forms with their three call schedules.
#include <algorithm>

#include "pamg_host.h"

using namespace pamg;
using namespace pamg::host;

namespace {

int rhs_level1(pamg_handle *h, int start_of_step) {
    Level &L = h->lv[1];
    Span sp(h, PAMG_K_RHS, (start_of_step == 1 ? 96.0 : start_of_step == 2 ? 72.0 : 48.0) * (double)L.N);
    HIPCHK(h, launch_rhs(h->stream, L, 1 / h->p.dt, start_of_step, PAMG_RHS_TOLD_HALO && start_of_step != 0));
    return PAMG_OK;
}

// restrictor(l) + get_residual(l) as one kernel (V-cycle driver)
int restrict_residual(pamg_handle *h, int l) {
    Level &L = h->lv[l];
    h->rhsn_valid = false;
    if (l >= h->p.multi_levels || h->p.op == 1) {
        CHK(restrict_(h, l));
        return residual(h, l);
    }
    if (l == 1 && h->p.solver == 2) CHK(rhs_level1(h, 0));   // get_RHS inside get_residual (:865-867)
    Span sp(h, PAMG_K_RESIDUAL, 102.0 * (double)L.N + 168.0 * h->U);
    HIPCHK(h, launch_restrict_residual(h->stream, L, h->lv[l + 1], 1 / h->p.dt));
    return PAMG_OK;
}

// algorithmic HBM bytes of the two fused V-cycle launches: the state each
// launch must read and write once, plus the operator words it reads (c, Kd, omega/D: 104 B
// per un_ele and level)
//   level-1 launch: level 1 reads tnew, RHS and writes residual, tnew, tnew_nonlin (120 B);
//                   level 2 reads the final tnew (prolongator) and writes RHSN (48 B)
//   coarse launch:  level l >= 2 reads tnew, RHSN and writes RHS, residual, tnew (120 B);
//                   RHSN of the levels l >= 3 is written here too (24 B)
double vcycle_fine_bytes(pamg_handle *h, int keep = PAMG_KEEP_ALL) {
    const int L = h->p.multi_levels;
    return (keep & PAMG_KEEP_L1 ? 120.0 : 72.0) * h->lv[1].N + (L > 1 ? 48.0 * h->lv[2].N : 0.0) + 104.0 * h->U;
}

double vcycle_coarse_bytes(pamg_handle *h, int keep = PAMG_KEEP_ALL) {
    const int L = h->p.multi_levels;
    double b = 0.0;
    for (int l = 2; l <= L; ++l) b += (120.0 - (keep & PAMG_KEEP_COARSE ? 0.0 : 48.0) + (l >= 3 ? 24.0 : 0.0)) * h->lv[l].N;
    return b + 104.0 * h->U * (L - 1);
}

//   pipelined launch: both, less level 2's RHSN (written and read: 48 B) and its tnew read
//                     by the coarse part (the level-1 part's read serves both: 24 B), less
//                     the dead-until-final stores it skips (keep, PAMG_KEEP_*): level 1's
//                     residual and tnew_nonlin (48 B), the coarse levels' RHS and residual
//                     (48 B); the halo words are not counted anywhere
double vcycle_pipe_bytes(pamg_handle *h, int keep) {
    double b = vcycle_fine_bytes(h) + vcycle_coarse_bytes(h) - 72.0 * h->lv[2].N;
    if (!(keep & PAMG_KEEP_L1)) b -= 48.0 * h->lv[1].N;
    if (!(keep & PAMG_KEEP_COARSE))
        for (int l = 2; l <= h->p.multi_levels; ++l) b -= 48.0 * h->lv[l].N;
    return b;
}

//   resident launch (a whole call): every level's state in and out once -- level 1 reads
//                     tnew and RHS (the source s' when it starts a step) and writes tnew,
//                     and with PAMG_KEEP_L1 its residual and tnew_nonlin (and the RHS it
//                     formed); told with PAMG_KEEP_TOLD; a coarse level reads tnew and RHSN
//                     and writes tnew and RHSN (level 2's RHSN: the restriction of level 1's
//                     last residual), with PAMG_KEEP_COARSE its RHS and residual
double vcycle_res_bytes(pamg_handle *h, int keep, bool rhsf) {
    const int L = h->p.multi_levels;
    double b = (72.0 + (keep & PAMG_KEEP_L1 ? (rhsf ? 72.0 : 48.0) : 0.0) + (keep & PAMG_KEEP_TOLD ? 24.0 : 0.0)) *
               h->lv[1].N;
    for (int l = 2; l <= L; ++l) b += (96.0 + (keep & PAMG_KEEP_COARSE ? 48.0 : 0.0)) * h->lv[l].N;
    return b + 104.0 * h->U * L;
}

// the stores a pipelined launch makes beyond what the call needs: none (forcing them, the round-2 A/B, moved
// 120 instead of 72 B per level-1 sub-element)
constexpr int kPipeKeep = 0;

// one V-cycle as the per-step kernel sequence of transport_tri_semi.F90:319-379
int vcycle_steps(pamg_handle *h) {
    const int L = h->p.multi_levels, ns = h->p.n_smooth;
    for (int l = 1; l <= L; ++l) {           // :323-340
        CHK(smooth(h, l, true, ns));
        CHK(restrict_residual(h, l));
    }
    if (h->p.coarse_solver == 1) CHK(direct_solve(h, L));   // the direct path instead of :344-359
    else CHK(smooth(h, L, true, ns * h->p.n_coarse));   // :344-359
    for (int l = L - 1; l >= 1; --l) {             // :363-378
        CHK(prolong(h, l, true));
        CHK(smooth(h, l, false, ns));
    }
    return PAMG_OK;
}

int vcycle_corrected(pamg_handle *h) {
    const int L = h->p.multi_levels, ns = h->p.n_smooth;
    h->overlap_static_l1 = false;   // the smoother calls rewrite the halo words
    for (int l = 1; l < L; ++l) {
        if (l > 1) HIPCHK(h, hipMemsetAsync(h->lv[l].T, 0, 3 * (size_t)h->lv[l].pitch * sizeof(double), h->stream));
        CHK(smooth_to_tnew(h, l, ns));
        CHK(residual_corrected(h, l));
        CHK(restrict_(h, l));
    }
    Level &C = h->lv[L];
    if (L > 1 && !h->agg) HIPCHK(h, hipMemsetAsync(C.T, 0, 3 * (size_t)C.pitch * sizeof(double), h->stream));   // a coarse level starts from zero
    if (h->agg) {
        CHK(agg_coarse_corrected(h));   // a partition: the agglomerated coarsest level
    } else if (L == 1) {
        CHK(smooth_to_tnew(h, 1, ns));
        CHK(residual_corrected(h, 1));
    } else if (h->p.coarse_solver == 1) {
        CHK(direct_solve(h, L));
    } else {
        CHK(smooth_to_tnew(h, L, ns * h->p.n_coarse));
    }
    for (int l = L - 1; l >= 1; --l) {
        {
            Span sp(h, PAMG_K_PROLONG, 216.0 * (double)h->lv[l + 1].N);
            HIPCHK(h, launch_interp_add(h->stream, h->lv[l], h->lv[l + 1]));
        }
        CHK(smooth_to_tnew(h, l, ns));
    }
    if (L > 1) CHK(residual_corrected(h, 1));   // the fine residual after the cycle
    h->tnn_level = 1;
    return PAMG_OK;
}

// the corrected cycle as one resident launch per pamg_vcycle call (pamg_vcycle_impl.h k_vc_corr): the
// call's cycles with every level of a tile on-chip, the state stored once at the end -- bitwise the
// per-step sequence above (tests/test_corrected.py). The halo words of the state are the last smoother
// call's, level 1's post-smoothing call of the last cycle (every coarser level writes a subset of its
// slots before it): its tnew words are written by the launch, the words constant within a time step by
// k_overlap_static, the remote ones exchanged after the call (halo_exchange = 0). fused = 0 keeps the per-step
// sequence.
bool corrected_resident_ok(pamg_handle *h) {
    return h->p.cycle == 1 && h->p.fused != 0 && h->p.op == 0 && h->p.coarse_solver == 0 && h->p.solver != 2 &&
           h->p.halo_exchange == 0 && h->p.n_smooth > 0 && call_schedule(h) == 3 &&
           vcycle_corrected_supported(h->p.n_split, h->p.multi_levels);
}

// algorithmic HBM bytes of the corrected resident call: level 1 reads tnew and RHS and writes tnew,
// tnew_nonlin and the residual (120 B); a level between writes RHS, residual, tnew, tnew_nonlin (96 B);
// the coarsest RHS, tnew, tnew_nonlin (72 B); the operator words (104 B per un_ele and level)
double vcycle_corr_bytes(pamg_handle *h) {
    const int L = h->p.multi_levels;
    double b = 120.0 * h->lv[1].N;
    for (int l = 2; l <= L; ++l) b += (l < L ? 96.0 : 72.0) * h->lv[l].N;
    return b + 104.0 * h->U * L;
}

// once per time step: the level-1 halo words the cycle's last smoother call leaves constant
// (t_overlap_old, the boundary words, the told halves of the send entries -- into both send buffers)
int overlap_static_once(pamg_handle *h) {
    if (h->overlap_static_l1) return PAMG_OK;
    HaloPlan &P1 = h->lv[1].halo;
    CHK(join_comm(h));
    HIPCHK(h, launch_overlap_static(h->stream, h->lv[1], h->U, h->tov, h->tovo, nullptr, h->told_halo_stale_l1));
    h->told_halo_stale_l1 = false;
    if (P1.d_send_b) HIPCHK(h, launch_overlap_static(h->stream, h->lv[1], h->U, h->tov, h->tovo, P1.d_send_b));
    h->overlap_static_l1 = true;
    return PAMG_OK;
}

// the send buffer a fused call packs (the alternate one where there are remote peers), once the exchange
// that read it has completed
int send_buf_take(pamg_handle *h, int *buf) {
    HaloPlan &P1 = h->lv[1].halo;
    *buf = P1.d_send_b ? 1 - P1.send_cur : 0;
    if (h->sent_pending[*buf]) {
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_sent[*buf], 0));
        h->sent_pending[*buf] = false;
    }
    return PAMG_OK;
}

// the end of a fused call that packed `buf`: its words exchanged -- dead: only send_cur advanced, the next
// call rewrites them unread -- and `stream` behind every exchange in flight
int send_buf_exchange(pamg_handle *h, int buf, bool dead) {
    if (dead) h->lv[1].halo.send_cur = buf;
    else CHK(halo_async(h, buf));
    return join_comm(h);
}

int vcycle_corrected_resident(pamg_handle *h, int n) {
    if (n <= 0) return PAMG_OK;
    const int L = h->p.multi_levels;
    HaloPlan &P1 = h->lv[1].halo;
    CHK(overlap_static_once(h));
    int buf = 0;
    CHK(send_buf_take(h, &buf));
    h->rhsn_valid = false;   // residuals and coarse RHS rewritten (RHSN does not follow them)
    {
        Span sp(h, PAMG_K_VCYCLE_CORR, vcycle_corr_bytes(h));
        HIPCHK(h, launch_vcycle_corrected(h->stream, h->lv, L, h->U, h->p.n_split, h->p.n_smooth, h->p.n_coarse,
                                          1 / h->p.dt, h->tov, h->tovo, P1.send_buf(buf), h->lv[2].RHSN, PAMG_KEEP_ALL, n));
    }
    h->tnn_level = 1;
    return send_buf_exchange(h, buf, false);
}

// schedule 3, resident: the call's n cycles in one launch (pamg_vcycle.hip k_vc_res), every
// tile's state on-chip between them; the final-cycle stores as the pipelined schedule makes
// them (the call's last launch stores all, or inside pamg_run the fields the next step reads)
int vcycle_fused_resident(pamg_handle *h, int n, bool dead_after, int steps, bool rhs_first) {
    const int L = h->p.multi_levels, ns = h->p.n_smooth;
    const double rdt = 1 / h->p.dt;
    HaloPlan &P1 = h->lv[1].halo;
    const bool two = P1.d_send_b != nullptr;   // remote peers: pack into alternate buffers
    Level &L2 = h->lv[2];
    int buf = 0;
    CHK(send_buf_take(h, &buf));
    const bool rhsf = rhs_first;
    const int kt = rhsf && !dead_after ? PAMG_KEEP_TOLD : 0;
    // inside pamg_run (dead_after) the halo words die unread too -- unless every cycle's are exchanged
    const bool hx = h->p.halo_exchange == 1;
    const int keep = (dead_after ? kPipeKeep | (hx ? PAMG_KEEP_HALO : 0) : PAMG_KEEP_ALL) | kt;
    if (kt) CHK(join_comm(h));   // the send buffers' told halves are rewritten
    // halo_exchange = 1: every cycle's words are exchanged. Cycles 0 .. n-2 pack the tnew words
    // of their remote entries into level 1's ring (k_vc_res / k_vc_resb with XC) and publish
    // each completed cycle on xc_sig; the comm stream waits for cycle c's count
    // (hipStreamWaitValue64) and exchanges it (exchange_ring) while the launch runs on; the last
    // cycle's words (6 per entry, with told) go as in the plain call, after the launch
    const bool xc = hx && n >= 2 && !P1.remote.empty();
    if (xc && (rhsf || steps != 1)) {
        h->err = "internal: a per-cycle exchange inside a resident time step";
        return PAMG_ERR_STATE;
    }
    if (xc) {
        CHK(xc_setup(h, n));
        HIPCHK(h, hipMemsetAsync(h->xc_done, 0, (size_t)(n - 1) * sizeof(unsigned), h->stream));
        {
            Span sp(h, PAMG_K_VCYCLE_RES, vcycle_res_bytes(h, keep, false) + 24.0 * (n - 1) * P1.remote.size());
            HIPCHK(h, launch_vcycle_resident_xc(h->stream, h->lv, L, h->U, h->p.n_split, ns, h->p.n_coarse, rdt,
                                                h->tov, h->tovo, P1.send_buf(buf), L2.RHSN, keep, n, P1.d_ring,
                                                3 * (int64_t)P1.remote.size(), h->xc_done, h->xc_sig));
        }
        if (h->comm && !P1.peers.empty())
            for (int c = 0; c + 1 < n; ++c) {
                HIPCHK(h, hipStreamWaitValue64(h->stream_comm, h->xc_sig, h->xc_sig_base + c + 1,
                                               hipStreamWaitValueGte));
                CHK(exchange_ring(h, c, h->stream_comm));
            }
        h->xc_sig_base += (unsigned long long)(n - 1);
    } else {
        // the per-call exchange, started early: the call's halo words are final once a tile has run its
        // last cycle, so the tiles with remote faces run first (tile order), count their ends, and the
        // last of them raises xc_sig; the comm stream waits on it and exchanges while the other tiles'
        // rounds run (the exchange reads only their send words and writes only the remote slots of
        // t_overlap / t_overlap_old, which no tile of the launch writes). A call that starts a time step
        // (RHSF) writes the send buffers' told halves itself and exchanges after the launch.
        const bool xe = !rhsf && !dead_after && steps == 1 && h->comm && !P1.peers.empty();
        EarlyXc X{};
        if (xe) {
            // the counter is never reset (a memset before the launch delays it by a few us): this call's
            // remote tiles complete it at the running total
            CHK(xe_setup(h));
            h->xe_total += (unsigned)h->xe_nremote;
            X = EarlyXc{h->xe_map, h->xe_done, h->xe_total, h->xc_sig};
        }
        const bool diag = xe && (h->timing.mask & (1u << PAMG_K_HALO_EARLY));
        if (diag) {
            for (auto &e : h->xe_ev)
                if (!e) HIPCHK(h, hipEventCreate(&e));
            HIPCHK(h, hipEventRecord(h->xe_ev[0], h->stream));
        }
        {
            Span sp(h, rhsf ? PAMG_K_VCYCLE_RES_RHSF : PAMG_K_VCYCLE_RES, vcycle_res_bytes(h, keep, rhsf));
            HIPCHK(h, launch_vcycle_resident(h->stream, h->lv, L, h->U, h->p.n_split, ns, h->p.n_coarse, rdt, h->tov,
                                             h->tovo, P1.send_buf(buf), L2.RHSN, keep, rhsf,
                                             two ? P1.send_buf(1 - buf) : nullptr, n, steps, xe ? &X : nullptr));
        }
        if (xe) {
            if (diag) HIPCHK(h, hipEventRecord(h->xe_ev[3], h->stream));
            HIPCHK(h, hipStreamWaitValue64(h->stream_comm, h->xc_sig, h->xc_sig_base + 1, hipStreamWaitValueGte));
            h->xc_sig_base += 1;
            if (diag) HIPCHK(h, hipEventRecord(h->xe_ev[1], h->stream_comm));
            {
                Span sp(h, PAMG_K_HALO_EARLY, 2.0 * 48.0 * (double)(P1.remote.size() + P1.recv_dst.size()),
                        h->stream_comm);
                CHK(exchange(h, 1, buf, h->stream_comm));
            }
            if (diag) {
                HIPCHK(h, hipEventRecord(h->xe_ev[2], h->stream_comm));
                h->xe_ev_valid = true;
            }
            HIPCHK(h, hipEventRecord(h->ev_sent[buf], h->stream_comm));
            h->sent_pending[buf] = true;
            P1.send_cur = buf;
            h->tnn_level = 1;
            // the join of `stream` behind the exchange is left to the next operation that needs it (settle,
            // at the entry of every other call; the next resident call waits only for the exchange that
            // read the send buffer it packs): a barrier packet behind the launch cost ~5-8 us of a 20-cycle
            // call at an N = 8 rank's shape (profiles/r05_i_xe_join.txt); pamg_synchronize waits for both
            return PAMG_OK;
        }
    }
    if (rhsf) {
        h->overlap_static_l1 = kt != 0;
        h->told_halo_stale_l1 = kt == 0;
    }
    h->tnn_level = 1;
    return send_buf_exchange(h, buf, dead_after && !hx);
}

// pipelined, halo exchanged once per call: the tiles are independent for the whole call
// (every operation is local to an un_ele, the halo words have no reader inside it), so two
// halves of them can run their launch sequences on two streams, each launch's drain
// overlapped by the other half's stream (schedule 2). Measured (scripts/ab_probe.py, profiles/r01_v16_tile_streams.txt):
// N = 4 partition 0.0404 -> 0.0339 ms per cycle, N = 8 0.0208 -> 0.0202, n_split = 3
// 0.0128 -> 0.0114, full mesh 0.1319 -> 0.1290. Automatic on partitions only: on one GPU
// the bench's per-launch events time launches, which schedule 2 overlaps.
//
// pamg_set_call_schedule(h, s): 0 automatic (3 where it applies, else 2 on a partition of
// a multi-rank run, 1 on one GPU), 1 one launch per cycle, 2 two tile streams, 3 resident
// (vcycle_fused_resident). (Round 1 tried a persistent
// form of the pipelined launch and dropped it at 128 VGPRs with spills; the resident form
// fits -- its final-cycle stores are peeled out of the cycle loop and its loop is
// unswitched by wave role, pamg_vcycle.hip k_vc_res / k_vc_resb.)
int vcycle_fused_streams(pamg_handle *h, int n, bool dead_after) {
    const int L = h->p.multi_levels, ns = h->p.n_smooth;
    const double rdt = 1 / h->p.dt;
    HaloPlan &P1 = h->lv[1].halo;
    Level &L2 = h->lv[2];
    const int tile = vcycle_tile_un_eles(h->p.n_split);
    const int ntiles = (h->U + tile - 1) / tile;
    int buf = 0;
    CHK(send_buf_take(h, &buf));
    const int mid = (ntiles / 2) * tile;
    HIPCHK(h, hipEventRecord(h->ev_fine, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream_c, h->ev_fine, 0));
    // launches alternate between the halves so that each stream always has the next one queued
    const hipStream_t st[2] = {h->stream, h->stream_c};
    // the first coarse launch's RHS and residual are rewritten by the first pipelined one
    const int ck = kPipeKeep & PAMG_KEEP_COARSE;
    const int ua[2] = {0, mid}, ub[2] = {mid, h->U};
    const int kf = dead_after ? kPipeKeep : PAMG_KEEP_ALL;   // the call's last level-1 launch
    for (int q = 0; q < 2; ++q) {
        Span sp(h, PAMG_K_VCYCLE_COARSE, vcycle_coarse_bytes(h, ck) * (ub[q] - ua[q]) / h->U, st[q]);
        HIPCHK(h, launch_vcycle_coarse(st[q], h->lv, L, h->U, h->p.n_split, ns, h->p.n_coarse, rdt, h->tov,
                                       h->tovo, L2.RHSN, ua[q], ub[q], ck));
    }
    for (int c = 0; c < n; ++c) {
        const bool pc = c + 1 < n;
        const int keep = pc ? kPipeKeep | (c + 2 == n && !dead_after ? PAMG_KEEP_COARSE : 0) : kf;
        for (int q = 0; q < 2; ++q) {
            const double f = (double)(ub[q] - ua[q]) / h->U;
            Span sp(h, pc ? PAMG_K_VCYCLE_PIPE : PAMG_K_VCYCLE,
                    f * (pc ? vcycle_pipe_bytes(h, keep) : vcycle_fine_bytes(h, keep)), st[q]);
            HIPCHK(h, launch_vcycle_fine(st[q], h->lv, L, h->U, h->p.n_split, ns, h->p.n_coarse, rdt, h->tov,
                                         h->tovo, P1.send_buf(buf), L2.RHSN, pc, keep, ua[q], ub[q]));
        }
    }
    HIPCHK(h, hipEventRecord(h->ev_coarse, h->stream_c));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_coarse, 0));
    h->tnn_level = 1;
    return send_buf_exchange(h, buf, dead_after);
}

// schedule 1, one launch per cycle (fused = 1, 2, 3)
int vcycle_fused_cycles(pamg_handle *h, int n, bool dead_after, bool rhs_first) {
    const int L = h->p.multi_levels, ns = h->p.n_smooth;
    const double rdt = 1 / h->p.dt;
    HaloPlan &P1 = h->lv[1].halo;
    const bool two = P1.d_send_b != nullptr;   // remote peers: pack into alternate buffers
    // fused = 2: the coarse launch of cycle c (levels 2..L, fp64-issue-bound) runs on stream_c
    // beside the level-1 launch of cycle c (HBM-bound). Their only shared data is level 2's
    // RHSN, read by the coarse launch and written by the level-1 launch: double-buffered,
    // so coarse(c) waits for level 1(c-1) (its RHS) and level 1(c) waits for coarse(c-1)
    // (the reader of the buffer it overwrites). The level-1 launch's prolongator (:370)
    // reads level 2's tnew, which coarse(c) may be rewriting: its result is dead (:550,
    // SURVEY.md A3 iv) and never stored, so no state depends on the order.
    const bool conc = h->p.fused == 2 && L > 1;
    // fused = 3: coarse(1), then [level 1 (c) + coarse levels (c+1)] for c < n, then level 1 (n)
    // (pamg_vcycle.hip, "pipelined tail"): nothing outside the call sees the coarse levels
    // one cycle ahead, and the last launch brings level 1 (and level 2's RHSN) level with them
    const bool pipe = h->p.fused == 3 && L > 1;
    Level &L2 = h->lv[2];
    if (conc) {
        HIPCHK(h, hipEventRecord(h->ev_fine, h->stream));   // everything issued before this call
    }
    // pamg_run: a step's last launch may have run this call's first coarse cycle already
    // (into_next below); else its RHS and residual stores are rewritten by the first
    // pipelined launch if n > 1
    if (pipe && n > 0 && !h->coarse_ahead) {
        const int ck = (n > 1 || dead_after) ? kPipeKeep & PAMG_KEEP_COARSE : PAMG_KEEP_ALL;
        Span sp(h, PAMG_K_VCYCLE_COARSE, vcycle_coarse_bytes(h, ck));
        HIPCHK(h, launch_vcycle_coarse(h->stream, h->lv, L, h->U, h->p.n_split, ns, h->p.n_coarse, rdt, h->tov,
                                       h->tovo, L2.RHSN, 0, -1, ck));
    }
    h->coarse_ahead = false;
    // pamg_run, every step but the last: the call's last level-1 launch is a pipelined one too,
    // carrying the next step's first coarse cycle -- it depends on this call's last residual
    // (:336) and on the coarse levels' own state only, not on begin_timestep (level 1) -- so
    // each step saves its separate coarse launch
    const bool into_next = pipe && dead_after && h->p.halo_exchange == 0;
    for (int c = 0; c < n; ++c) {
        int buf = 0;
        CHK(send_buf_take(h, &buf));   // the exchange that read this buffer two cycles ago
        double *rhsn_w = conc ? (L2.RHSN == L2.RHSN_alt ? L2.T + 15 * L2.pitch : L2.RHSN_alt) : L2.RHSN;
        if (conc) {
            HIPCHK(h, hipStreamWaitEvent(h->stream_c, h->ev_fine, 0));
            if (c > 0) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_coarse, 0));
        }
        if (L > 1 && !pipe) {   // levels 2..L first: the prolongator of level 1 reads their final tnew
            const hipStream_t sc = conc ? h->stream_c : h->stream;
            Span sp(h, PAMG_K_VCYCLE_COARSE, vcycle_coarse_bytes(h), sc);
            HIPCHK(h, launch_vcycle_coarse(sc, h->lv, L, h->U, h->p.n_split, ns, h->p.n_coarse, rdt, h->tov,
                                           h->tovo, L2.RHSN));
            if (conc) HIPCHK(h, hipEventRecord(h->ev_coarse, h->stream_c));
        }
        {
            const bool pc = pipe && (c + 1 < n || into_next);   // also the coarse levels of cycle c + 1
            // its stores that the rest of the call overwrites unread are skipped: level 1's
            // residual and tnew_nonlin always (the call's last launch is k_vc_fine, which stores
            // them), the coarse levels' RHS and residual unless they reach their final cycle
            // here, the halo words unless every cycle's are exchanged
            const bool dead = pipe && dead_after && h->p.halo_exchange == 0;
            const int keep = c + 1 == n && into_next ? kPipeKeep | (n == 1 ? PAMG_KEEP_COARSE : 0)
                             : pc ? kPipeKeep | (c + 2 == n && !dead ? PAMG_KEEP_COARSE : 0) |
                                        (h->p.halo_exchange == 1 ? PAMG_KEEP_HALO : 0)
                                  : (dead && c + 1 == n ? kPipeKeep : PAMG_KEEP_ALL);
            // rhs_first: this launch also starts the time step -- told := tnew and level 1's RHS
            // (k_rhs's work: +48 B stored, 24 B of RHS not read per level-1 sub-element)
            // (+24 B of s' read and 24 B of RHS stored per level-1 sub-element, the RHS read
            // saved; kKeepTold, the step the next one does not overwrite: told stored and the
            // step's constant halo words written, k_overlap_static's work)
            const bool rhsf = rhs_first && c == 0;
            if (rhsf && !pc) { h->err = "internal: time-step start on a non-pipelined launch"; return PAMG_ERR_STATE; }
            const int kt = rhsf && !dead_after ? PAMG_KEEP_TOLD : 0;
            Span sp(h, rhsf ? PAMG_K_VCYCLE_RHSF : pc ? PAMG_K_VCYCLE_PIPE : PAMG_K_VCYCLE,
                    (pc ? vcycle_pipe_bytes(h, keep) : vcycle_fine_bytes(h, keep)) +
                        (rhsf ? (kt ? 48.0 : 24.0) * h->lv[1].N : 0.0));
            if (kt) CHK(join_comm(h));   // the send buffers' told halves are rewritten
            HIPCHK(h, launch_vcycle_fine(h->stream, h->lv, L, h->U, h->p.n_split, ns, h->p.n_coarse, rdt, h->tov,
                                         h->tovo, P1.send_buf(buf), L > 1 ? rhsn_w : nullptr, pc, keep | kt, 0, -1,
                                         rhsf, two ? P1.send_buf(1 - buf) : nullptr));
            if (rhsf) {
                // kKeepTold: the launch wrote what k_overlap_static would (from told in registers);
                // else told and those words are dead until the next step rewrites them
                h->overlap_static_l1 = kt != 0;
                h->told_halo_stale_l1 = kt == 0;
            }
            if (conc) HIPCHK(h, hipEventRecord(h->ev_fine, h->stream));
        }
        if (L > 1) L2.RHSN = rhsn_w;   // the next cycle's level-2 RHS
        h->tnn_level = 1;
        // every halo word of the cycle was written by the level-1 launch (its remote ones
        // packed into `buf`); the next cycle rewrites every one of them and nothing reads
        // t_overlap in between: halo_exchange = 0 exchanges the last cycle's words only,
        // 1 every cycle's, in flight during the next one
        if (h->p.halo_exchange == 1 || (c + 1 == n && !(pipe && dead_after))) CHK(halo_async(h, buf));
        else if (c + 1 == n) P1.send_cur = buf;
    }
    h->coarse_ahead = into_next && n > 0;
    if (conc && n > 0) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_coarse, 0));   // join
    return join_comm(h);
}

}  // namespace

namespace pamg {
namespace host {

// `sweeps` sweeps on level l reading the iterate from T (src_is_T: the leg
// copy tnew_nonlin := tnew is folded into the launch) or from TNN.
int smooth(pamg_handle *h, int l, bool src_is_T, int sweeps) {
    Level &L = h->lv[l];
    h->tnn_level = l;
    h->overlap_static_l1 = false;   // the per-step smoother writes every halo word of level l
    if (sweeps <= 0) {
        if (src_is_T) HIPCHK(h, launch_copy(h->stream, L.T, L.TNN, 3 * L.pitch));
        return PAMG_OK;
    }
    const double rdt = 1 / h->p.dt;
    const int kid = (l == 1) ? PAMG_K_SMOOTH_L1 : PAMG_K_SMOOTH;
    const double bytes = 96.0 * (double)L.N + 168.0 * h->U;
    if (h->p.op == 1) {   // face-coupled operator: the halo is read, so it is refreshed (and exchanged) every sweep
        // the tile launches: one per sweep, or the whole call in one (face_call)
        if (face_tiles_ok(h, l)) return face_call(h, l, src_is_T, sweeps, false);
        if (src_is_T) HIPCHK(h, launch_copy(h->stream, L.T, L.TNN, 3 * L.pitch));
        // a partition: per sweep the halo refresh, the exchange, then the sweep itself -- one tile
        // launch (both colours on the iterate in LDS, reading the exchanged t_overlap) or the two
        // colour kernels
        const bool tiles = face_tiles_ok(h, l);
        for (int s = 0; s < sweeps; ++s) {
            HIPCHK(h, launch_face_halo(h->stream, L, h->tov, h->tovo, true));   // tnew := tnew_nonlin (:550), :555
            CHK(halo(h, l));
            Span sp(h, kid, tiles ? 72.0 * (double)L.N + 168.0 * h->U : bytes + 72.0 * (double)L.N);
            if (tiles) {   // tnew_nonlin only: the refresh has copied tnew := tnew_nonlin
                HIPCHK(h, launch_face_sweep_fused(h->stream, L, h->tov, nullptr, h->tovo, h->p.solver == 3, l == 1, rdt,
                                                  h->p.omega, h->slots, 0, false));
            } else if (h->p.solver == 3) {   // red-black Gauss-Seidel: up sub-elements, then down ones
                HIPCHK(h, launch_face_sweep(h->stream, L, h->tov, 0, l == 1, rdt, h->p.omega, h->slots));
                HIPCHK(h, launch_face_sweep(h->stream, L, h->tov, 1, l == 1, rdt, h->p.omega, h->slots));
            } else {
                HIPCHK(h, launch_face_sweep(h->stream, L, h->tov, 2, l == 1, rdt, h->p.omega, h->slots));
            }
        }
        return PAMG_OK;
    }
    if (h->p.halo_mode == 1) {
        for (int s = 0; s < sweeps; ++s) {
            {
                Span sp(h, kid, bytes);
                HIPCHK(h, launch_smooth(h->stream, L, (s == 0 && src_is_T) ? L.T : L.TNN, 1, h->p.solver, rdt,
                                        h->p.omega, h->tov, h->tovo));
            }
            CHK(halo(h, l));
        }
        return PAMG_OK;
    }
    {
        Span sp(h, kid, bytes);
        HIPCHK(h, launch_smooth(h->stream, L, src_is_T ? L.T : L.TNN, sweeps, h->p.solver, rdt, h->p.omega, h->tov,
                                h->tovo));
    }
    return halo(h, l);
}

// told changed on level l: refresh the compact told copy the halo reads
int refresh_told_halo(pamg_handle *h, int l) {
    h->overlap_static_l1 = false;
    if (l == 1) h->told_halo_stale_l1 = false;
    HIPCHK(h, launch_told_halo(h->stream, h->lv[l], h->U));
    return PAMG_OK;
}

int residual(pamg_handle *h, int l) {
    Level &L = h->lv[l];
    if (h->p.op == 1) return face_residual(h, l, false);
    h->rhsn_valid = false;
    if (l == 1 && h->p.solver == 2) CHK(rhs_level1(h, 0));   // get_RHS inside get_residual (:865-867)
    Span sp(h, PAMG_K_RESIDUAL, 72.0 * (double)L.N + 168.0 * h->U);
    HIPCHK(h, launch_residual(h->stream, L, 1 / h->p.dt));
    return PAMG_OK;
}

int restrict_(pamg_handle *h, int l) {
    if (l >= h->p.multi_levels) return PAMG_OK;   // splitting.F90:18
    Span sp(h, PAMG_K_RESTRICT, 96.0 * (double)h->lv[l + 1].N);
    HIPCHK(h, launch_restrict(h->stream, h->lv[l], h->lv[l + 1], h->U));
    return PAMG_OK;
}

int prolong(pamg_handle *h, int l, bool fused_copy) {
    if (l >= h->p.multi_levels) { h->err = "prolongator needs a coarser level"; return PAMG_ERR_ARG; }
    if (fused_copy) h->tnn_level = l;
    Span sp(h, PAMG_K_PROLONG, (fused_copy ? 312.0 : 216.0) * (double)h->lv[l + 1].N);
    HIPCHK(h, launch_prolong(h->stream, h->lv[l], h->lv[l + 1], fused_copy));
    return PAMG_OK;
}

// fp64 operations one V-cycle of the fused forms executes (fma = 2): a sweep is 12 fma (24 flop,
// contracted) or 42 operations (the reference's order, apply_A + update), get_residual 9 fma or
// 36; the restrictor's input mean 3 per sub-element of the levels < L; the prolongator cascade 21
// per coarse sub-element (splitting.F90:59-88, executed on LDS images although its output is dead).
// A smoother call's last sweep only produces tnew_nonlin; inside a fused cycle that value is
// overwritten before any read (:367 after the restriction leg, :327 of the next cycle after the
// prolongation leg, :348 on the coarsest level), so it is never computed (the compiler drops it:
// its result never leaves registers) -- per cycle a level l < L runs 2 (n_smooth - 1) sweeps and
// the coarsest n_smooth (1 + n_coarse) - 2; only a call's last cycle also runs level 1's final
// sweep, whose tnew_nonlin it stores (not counted here)
double vcycle_flops(pamg_handle *h) {
    const int L = h->p.multi_levels, ns = h->p.n_smooth, nc = h->p.n_coarse;
    const bool f = h->p.arith == 1 && h->p.solver != 2;
    // Richardson's update is x + omega b (a multiply and an add per component), its residual the
    // reference's order
    const double sw = h->p.solver == 2 ? 6.0 : f ? 24.0 : 42.0, rs = f ? 18.0 : 36.0;
    if (h->p.cycle == 1) {
        // the corrected cycle: every sweep is live -- a level l < L runs two calls of n_smooth sweeps, the
        // fresh residual and its mean (3), and takes the interpolated correction (3 adds per sub-element,
        // the three midpoints, 9 flops, per coarse parent); the coarsest n_coarse calls from zero; the fine
        // residual after the cycle only in a call's last cycle (not counted)
        double fl = 0.0;
        for (int l = 1; l <= L; ++l) {
            const double n = (double)h->lv[l].N;
            if (l < L) fl += n * (2.0 * ns * sw + rs + 3.0 + 3.0) + 9.0 * (double)h->lv[l + 1].N;
            else fl += n * ((double)ns * (L > 1 ? nc : 1) * sw + (L > 1 ? 0.0 : rs));
        }
        return fl;
    }
    // the resident kernels (call schedule 3) do not compute the dead prolongator (pamg_vcycle.hip
    // k_vc_res, k_vc_resb); every other fused form executes its cascade
    const bool prolong = !(call_schedule(h) == 3 && vcycle_resident_supported(h->p.n_split, L));
    double fl = 0.0;
    for (int l = 1; l <= L; ++l) {
        const double n = (double)h->lv[l].N;
        if (l < L) fl += n * (2.0 * std::max(ns - 1, 0) * sw + rs + 3.0);
        else fl += n * ((nc > 0 ? (double)ns * (1 + nc) - 2 : (double)ns - 1) * sw + rs);
        if (l >= 2 && prolong) fl += n * 21.0;
    }
    return fl;
}

// the exact local solve of level l (coarse_solver = 1): tnew = tnew_nonlin = A_e^-1 RHS, with
// A_e^-1 from FINDInv, formed on first use
int direct_solve(pamg_handle *h, int l) {
    Level &L = h->lv[l];
    if (!L.Ainv) {
        int *d_err = nullptr;
        CHK(dev_alloc(h, &L.Ainv, 9 * (size_t)std::max(h->U, 1)));
        HIPCHK(h, hipMalloc((void **)&d_err, sizeof(int) * std::max(h->U, 1)));
        HIPCHK(h, launch_block_ops(h->stream, L, h->U, 1 / h->p.dt, L.Ainv, d_err));
        std::vector<int> err(std::max(h->U, 1));
        HIPCHK(h, hipMemcpyAsync(err.data(), d_err, sizeof(int) * h->U, hipMemcpyDeviceToHost, h->stream));
        CHK(sync_stream(h, h->stream));   // (the gates first: hipFree waits for the whole device)
        (void)hipFree(d_err);
        for (int q = 0; q < h->U; ++q)
            if (err[q]) {
                h->err = "FINDInv: operator block of un_ele " + std::to_string(h->owned[q] + 1) + " on level " +
                         std::to_string(l) + " is not invertible";
                return PAMG_ERR_STATE;
            }
    }
    h->tnn_level = l;
    HIPCHK(h, launch_block_solve(h->stream, L, L.Ainv));
    return PAMG_OK;
}

// the corrected V-cycle (params.cycle = 1; oracle orc_vcycle_corrected):
// the reference's smoother, restrictor and levels with the cycle's defects fixed -- the
// restrictor acts on the fresh residual b - A x, coarse levels start from zero, the prolonged
// correction is added to the iterate the next smoother call starts from. A level's iterate
// after a smoother call is its tnew_nonlin (the last sweep), copied to tnew.
int smooth_to_tnew(pamg_handle *h, int l, int sweeps) {
    Level &L = h->lv[l];
    CHK(smooth(h, l, true, sweeps));
    HIPCHK(h, launch_copy(h->stream, L.TNN, L.T, 3 * L.pitch));
    return PAMG_OK;
}

int residual_corrected(pamg_handle *h, int l) {
    if (h->p.op == 1) return face_residual(h, l, true);
    h->rhsn_valid = false;
    Span sp(h, PAMG_K_RESIDUAL, 72.0 * (double)h->lv[l].N + 168.0 * h->U);
    HIPCHK(h, launch_residual(h->stream, h->lv[l], 1 / h->p.dt, true));
    return PAMG_OK;
}

// n V-cycles as two fused launches each (pamg_vcycle.hip)
// pipelined-call schedule (pamg_set_call_schedule)
// 0 automatic: the resident form where it applies (two levels or more, the halo words exchanged
// once per call), else one launch per cycle (one GPU) or two tile streams (a partition)
int call_schedule(pamg_handle *h) {
    const int s = h->call_schedule;
    if (s) return s;
    if (vcycle_resident_supported(h->p.n_split, h->p.multi_levels)) return 3;
    return h->nranks > 1 ? 2 : 1;
}

// the fused forms of the V-cycle apply; Richardson (solver 2) has its update only in the resident
// call (pamg_vcycle.hip k_vc_res with StcR), so it is fused there and nowhere else
bool fused_ok(pamg_handle *h) {
    const int L = h->p.multi_levels;
    if (!(h->p.fused && h->p.cycle == 0 && h->p.coarse_solver == 0 && h->p.op == 0 &&
          vcycle_fusable(h->lv, L, h->p.n_split, h->p.solver, h->p.halo_mode, h->p.n_smooth)))
        return false;
    if (h->p.solver != 2) return true;
    return h->p.fused == 3 && call_schedule(h) == 3 && !h->coarse_ahead && vcycle_resident_supported(h->p.n_split, L);
}

// dead_after (pamg_run, every step but the last): the next call rewrites the fields this one
// leaves for an observer -- level 1's residual and tnew_nonlin, the coarse levels' RHS and
// residual, the halo words -- before any read (nothing reads t_overlap, the next step's first
// restrictor reads level 2's RHSN, which is stored), so the pipelined schedule skips them
// and the exchange of the halo words too
// steps > 1: the resident schedule runs `steps` time steps of n cycles in one launch (pamg_run;
// the call starts the first step, rhs_pending)
int vcycle_fused(pamg_handle *h, int n, bool dead_after, int steps) {
    const int L = h->p.multi_levels;
    if (!h->rhsn_valid) {   // residuals changed outside the fused cycle: restrict them afresh
        for (int l = 1; l < L; ++l)
            HIPCHK(h, launch_restrict(h->stream, h->lv[l], h->lv[l + 1], h->U, h->lv[l + 1].RHSN));
        h->rhsn_valid = true;
    }
    // once per time step: the halo words the cycle's last smoother leaves constant (into both
    // send buffers); when this call starts a pamg_run step whose told and RHS its first level-1
    // launch computes (rhs_pending), after that launch, as it reads told
    const bool rhs_first = h->rhs_pending;
    h->rhs_pending = false;
    if (!rhs_first) CHK(overlap_static_once(h));
    const bool pipe = h->p.fused == 3 && L > 1;
    const int sched = call_schedule(h);
    if (steps > 1 && !(pipe && n >= 1 && sched == 3 && h->p.halo_exchange == 0 && !h->coarse_ahead && rhs_first &&
                       vcycle_resident_run_supported(h->p.n_split, L))) {
        h->err = "internal: a resident run outside the resident schedule";
        return PAMG_ERR_STATE;
    }
    if (h->p.solver == 2 && n >= 1 &&
        !(pipe && sched == 3 && !h->coarse_ahead && vcycle_resident_supported(h->p.n_split, L))) {
        h->err = "internal: Richardson outside the resident call";
        return PAMG_ERR_STATE;
    }
    if (pipe && n >= 1 && sched == 3 && !h->coarse_ahead && vcycle_resident_supported(h->p.n_split, L))
        return vcycle_fused_resident(h, n, dead_after, steps, rhs_first);
    const int tile = vcycle_tile_un_eles(h->p.n_split);
    const int ntiles = (h->U + tile - 1) / tile;
    if (pipe && n > 1 && sched == 2 && h->p.halo_exchange == 0 && ntiles >= 2 && !h->coarse_ahead)
        return vcycle_fused_streams(h, n, dead_after);
    return vcycle_fused_cycles(h, n, dead_after, rhs_first);
}

// tnn_dead: the caller runs a V-cycle next, whose first smoother call rewrites tnew_nonlin
// (:327) before any read, so the :317 copy is not stored (pamg_run); told_lazy: that V-cycle
// is the fused one, whose k_overlap_static refreshes the compact told copy of the halo from
// TOLD itself (one launch instead of k_told_halo + k_overlap_static)
int begin_timestep(pamg_handle *h, bool tnn_dead, bool told_lazy, bool defer_rhs) {
    CHK(check_level(h, 1));
    // the first launch of the step's fused V-cycle does k_rhs's work (Richardson: the resident
    // launch, which also rebuilds the RHS where get_residual does)
    if (defer_rhs && (h->p.solver != 2 || fused_ok(h))) {
        h->tnn_level = 1;
        h->overlap_static_l1 = false;
        h->told_halo_stale_l1 = true;
        h->rhs_pending = true;
        return PAMG_OK;
    }
    h->tnn_level = 1;
    if (h->p.solver == 2) {   // solve_Richardson never calls get_RHS inside the smoother
        Level &L = h->lv[1];
        HIPCHK(h, launch_copy(h->stream, L.T, L.TOLD, 3 * L.pitch));
        HIPCHK(h, launch_copy(h->stream, L.T, L.TNN, 3 * L.pitch));
        return refresh_told_halo(h, 1);
    }
    CHK(rhs_level1(h, tnn_dead ? 2 : 1));   // also the compact told copy of the halo (refresh_told_halo)
    if (PAMG_RHS_TOLD_HALO || told_lazy) {
        h->overlap_static_l1 = false;
        h->told_halo_stale_l1 = !PAMG_RHS_TOLD_HALO;
        return PAMG_OK;
    }
    return refresh_told_halo(h, 1);
}

int vcycle(pamg_handle *h, int n, bool dead_after) {
    CHK(check_level(h, 1));
    // no pass of the loop body (:319): nothing is written -- not the step's constant halo words, which the
    // fused forms put back before their first cycle, and not tnn_level, which every form sets after its last
    if (n == 0) return PAMG_OK;
    // the fused op = 0 forms wait only for the exchange that read the send buffer they pack; the others may
    // touch anything an early exchange still in flight touches
    if (!(h->p.cycle == 0 && fused_ok(h))) CHK(settle(h));
    if (h->p.cycle == 1) {
        if (corrected_resident_ok(h)) return vcycle_corrected_resident(h, n);
        if (face_corrected_pp_ok(h)) return vcycle_corrected_face_pp(h, n);
        for (int c = 0; c < n; ++c) CHK(vcycle_corrected(h));
        return h->p.op == 1 ? face_chain_check(h) : PAMG_OK;
    }
    if (fused_ok(h)) return vcycle_fused(h, n, dead_after);
    if (face_cycle_fusable(h)) return vcycle_face_fused(h, n);
    for (int c = 0; c < n; ++c) CHK(vcycle_steps(h));
    return h->p.op == 1 ? face_chain_check(h) : PAMG_OK;
}

}  // namespace host
}  // namespace pamg
