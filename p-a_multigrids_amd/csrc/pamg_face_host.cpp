// The host side of the face-coupled operator (op = 1): the smoother call (persistent chain, gates,
// one launch per sweep), the two-sweep passes, the agglomerated coarsest level of a partition, the
// fused and corrected face cycles, and the convergence monitor's buffers and exchange.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "pamg_host.h"

using namespace pamg;
using namespace pamg::host;

namespace {

// the device's compute-unit count, read on first use
int device_cus(pamg_handle *h) {
    if (!h->cus) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || n <= 0) n = 1;
        h->cus = n;
    }
    return h->cus;
}

// the face-coupled operator's smoother call on a single domain, one launch per sweep
// (k_face_sweep): the halo snapshots alternate between two t_overlap buffers so that a sweep's
// halo words for the next sweep never overwrite the ones it reads; the call's last sweep reads
// h->tov, which therefore holds the words of its start, as after the per-colour sequence.
// dead_last (the fused face V-cycle, vcycle_face_fused): the call's last sweep only produces a
// tnew_nonlin that the cycle overwrites unread (:327, :348, :367) -- it is not run; the sweep before
// it stores its result as tnew (the dead sweep's :550) and writes the dead sweep's :555 words into
// h->tov, so tnew and t_overlap are what the full call leaves.
// the persistent chain (pamg_face.hip k_face_chain) for a smoother call of level l: a single
// domain whose level fits one workgroup per CU (face_chain_fits); PAMG_FACE_CHAIN=0 turns it off
bool face_chain_ok(pamg_handle *h, int l) {
    const char *ev = getenv("PAMG_FACE_CHAIN");   // read per call: tests switch it within a process
    if ((ev && atoi(ev) == 0) || h->nranks != 1 || h->comm || h->neig_local.empty()) return false;
    // the coarsest-level replica of a partition in a local group (pamg_comm_local_group: every rank's handle in
    // one process, on one GPU): the ranks' chains would compete for the same CUs, and an aborted one's fallback
    // (the host's launches on stream_fb) can sit behind another rank's gate in a shared hardware queue -- such a
    // replica runs its calls one launch per sweep (bitwise the chain). One process per GPU keeps the chain.
    if (h->tparent && h->tparent->comm && h->tparent->comm->local) return false;
    return face_chain_fits(h->lv[l].nsub, h->U, device_cus(h));
}

// its neighbour lists: workgroup w owns un_eles [w k, (w+1) k); its neighbours are the other
// workgroups owning a neighbour of one of them (they write the halo words w reads)
int face_chain_setup(pamg_handle *h, int l) {
    Level &L = h->lv[l];
    if (L.chain_g) return PAMG_OK;
    const int U = h->U, g0 = std::max(1, std::min(h->cus, U)), k = (U + g0 - 1) / g0, G = (U + k - 1) / k;
    std::vector<int> off(1, 0), list;
    for (int w = 0; w < G; ++w) {
        std::vector<int> nb;
        for (int q = w * k; q < std::min(U, (w + 1) * k); ++q)
            for (int f = 0; f < 3; ++f) {
                const int n = h->neig_local[3 * (size_t)q + f];
                if (n >= 0 && n / k != w) nb.push_back(n / k);
            }
        std::sort(nb.begin(), nb.end());
        nb.erase(std::unique(nb.begin(), nb.end()), nb.end());
        list.insert(list.end(), nb.begin(), nb.end());
        off.push_back((int)list.size());
    }
    if (list.empty()) list.push_back(0);
    CHK(dev_upload(h, &L.chain_nb_off, off));
    CHK(dev_upload(h, &L.chain_nb_list, list));
    // the polled words in one block of their own, a multiple of 16 bytes from the allocation's start: one
    // per workgroup (k_face_chain) or per wave of it (k_face_chain_pw, 16 a workgroup)
    L.chain_flag_bytes = ((size_t)G * 16 * sizeof(unsigned) + 15) / 16 * 16;
    CHK(dev_alloc(h, &L.chain_flags, L.chain_flag_bytes / sizeof(unsigned)));
    HIPCHK(h, hipMemsetAsync(L.chain_flags, 0, L.chain_flag_bytes, h->stream));
    L.chain_epoch = 0;
    if (!h->chain_tmo) {
        CHK(dev_alloc(h, &h->chain_tmo, 4));
        HIPCHK(h, hipMemsetAsync(h->chain_tmo, 0, 4 * sizeof(unsigned), h->stream));
    }
    L.chain_g = G;
    return PAMG_OK;
}

// face_call's executed sweeps as one launch each (from the snapshot the call's halo refresh wrote)
int face_call_sweeps(pamg_handle *h, int l, int sweeps, int run, bool dead_last, bool src_is_T, bool both, bool res_in_sweep) {
    Level &L = h->lv[l];
    const double rdt = 1 / h->p.dt;
    const int kid = (l == 1) ? PAMG_K_SMOOTH_L1 : PAMG_K_SMOOTH;
    double *buf[2] = {h->tov, h->tov_b};
    for (int s = 0; s < run; ++s) {
        const bool fin = s + 1 == run;
        // read tnew_nonlin, RHS; write tnew_nonlin (+ tnew in the last sweep, + the next halo words)
        const int store = fin ? (dead_last ? 2 : 1) : 0;
        const bool r = s == 0 && res_in_sweep;
        if (r) h->rhsn_valid = false;
        Span sp(h, kid, (store == 1 ? 96.0 : 72.0) * (double)L.N + (r ? 24.0 * (double)L.N : 0.0) + 168.0 * h->U);
        HIPCHK(h, launch_face_sweep_fused(h->stream, L, buf[(sweeps - 1 - s) & 1],
                                          s + 1 < sweeps ? buf[(sweeps - 2 - s) & 1] : nullptr, h->tovo,
                                          h->p.solver == 3, l == 1, rdt, h->p.omega, h->slots, store, s == 0,
                                          s == 0 && src_is_T, r ? L.RES : nullptr));
        if (s + 1 < sweeps) CHK(halo(h, l, buf[(sweeps - 2 - s) & 1]));   // the next sweep's remote words
    }
    if (both) HIPCHK(h, launch_copy(h->stream, L.TNN, L.T, 3 * L.pitch));
    return PAMG_OK;
}

int face_gate_setup(pamg_handle *h) {
    if (h->gate) return PAMG_OK;
    // the stream waits on it (hipStreamWaitValue64): HIP's signal memory, as xc_sig
    HIPCHK(h, hipExtMallocWithFlags((void **)&h->gate, sizeof(unsigned long long), hipMallocSignalMemory));
    unsigned long long v = 0;
    HIPCHK(h, hipMemcpy(&v, h->gate, sizeof v, hipMemcpyDeviceToHost));
    h->gate_base = v;
    HIPCHK(h, hipHostMalloc((void **)&h->gate_stat, kGateRing * sizeof(unsigned long long), hipHostMallocCoherent));
    memset(h->gate_stat, 0, kGateRing * sizeof(unsigned long long));   // (tags start at 1)
    HIPCHK(h, hipStreamCreateWithFlags(&h->stream_fb, hipStreamNonBlocking));
    return PAMG_OK;
}

// ---- the face V-cycle with two sweeps per HBM pass (k_face_pp) on the levels below the coarsest
// The fused cycle's level-l work, for l < L, is a stream of sweeps on one RHS: its restriction-leg call's
// executed sweeps and its prolongation-leg call's, which starts from the restriction-leg tnew (:367; the
// prolongated values are overwritten unread, :550), with get_residual between them -- and level 1's RHS
// is the time step's, so level 1's streams of all the call's cycles are ONE stream (its coarse levels
// never feed back into it). Such a stream runs as launches of two sweeps (the halo of the second sweep
// computed in the launch, k_face_pp), the residual inside the launch that passes its point, and the
// state rotating through tnew, tnew_nonlin and RHSN (op = 1 has no use for RHSN) -- a launch never writes
// the iterate its neighbours read. The restrictor of level l (:336, the PREVIOUS residual) runs before the
// launch that writes the new one; a coarse level's whole cycle runs before the next level's (nothing of
// the next level reaches it). The halo words (:555) are no longer published between sweeps (the launches
// read the iterate itself): t_overlap, t_overlap_old and the boundary words are written from level 1's
// tnew once, after the call -- what the per-step sequence's last writer, level 1's last smoother call,
// leaves (every coarser level writes a subset of its slots). Bitwise the per-step sequence
// (tests/test_face_operator.py). PAMG_FACE_PP=0 keeps the one-sweep launches (A/B).
// PAMG_FACE_PP: a mask of the level sizes that stream -- bit 0 levels of 1,024 sub-elements per un_ele,
// bit 1 of 256; 0 none. Default 3: both (the 256-element passes were slower while their instance
// spilled at six waves per SIMD, profiles/r04_d_face_pp.txt; at four, 620 vs 601-603 V-cycles/s with
// level 1 alone, profiles/r04_i_face_pp_level2.txt)
bool face_pp_ok(pamg_handle *h, int l) {
    const char *ev = getenv("PAMG_FACE_PP");   // read per call: tests switch it within a process
    const int mask = ev ? atoi(ev) : 3;
    const Level &L = h->lv[l];
    const int bit = L.nsub == 1024 ? 1 : L.nsub == 256 ? 2 : 0;
    // a single domain: the passes read the neighbours' iterate itself
    return (mask & bit) && face_tiles_ok(h, l) && h->nranks == 1 && !h->comm && face_tile_shape(L) && L.gtab &&
           (h->p.solver != 3 || L.words_up);
}

// a pass of a face stream (face_pp_plan); rhsc: its residual also restricted into this buffer (res_drop: and not
// stored), interp: the coarse correction added to its loads (PPCoarse)
struct PPPass {
    int K, res;
    double *in, *pre, *mid, *end, *end2;
    bool interp = false;
    double *rhsc = nullptr;
    bool res_drop = false;
};

// the passes of a stream of `total` sweeps from src with get_residual after sweep r for each r in res_at
// (0 < r < total), ending with the final stores fin (1: tnew = the iterate before the last sweep,
// tnew_nonlin = after it; 2: tnew = the last result, the dead sweep's :550; 3: tnew and tnew_nonlin both
// the last result, the corrected cycle's smoother call)
int face_pp_plan(pamg_handle *h, int l, int total, double *src, const std::vector<int> &res_at, int fin,
                 std::vector<PPPass> &plan) {
    Level &L = h->lv[l];
    plan.clear();
    for (int s = 0; s < total; s += 2)
        plan.push_back(PPPass{std::min(2, total - s), 0, nullptr, nullptr, nullptr, nullptr, nullptr});
    for (int r : res_at) {
        if (r <= 0 || r >= total) { h->err = "internal: face stream residual point"; return PAMG_ERR_STATE; }
        PPPass &q = plan[r / 2];
        if (q.res) { h->err = "internal: two residuals in one face pass"; return PAMG_ERR_STATE; }
        q.res = (r & 1) ? 2 : 1;   // after the pass's first sweep, or at its start
    }
    const int P = (int)plan.size();
    PPPass &z = plan[P - 1];
    if (fin == 1) {
        if (z.K == 2) z.mid = L.T; else z.pre = L.T;
        z.end = L.TNN;
    } else {
        z.end = L.T;
        if (fin == 3) z.end2 = L.TNN;
    }
    double *const buf[3] = {L.RHSN, L.TNN, L.T};
    // inputs, last to first: the last pass reads RHSN (neither of its outputs); every other pass writes the
    // next one's input, which is not its own; the first reads src
    std::vector<double *> in(P);
    in[P - 1] = P == 1 ? src : L.RHSN;
    for (int p = P - 2; p >= 1; --p)
        for (double *b : buf)
            if (b != in[p + 1] && (p != 1 || b != src)) { in[p] = b; break; }
    if (P >= 2) in[0] = src;
    for (int p = 0; p < P; ++p) {
        plan[p].in = in[p];
        if (p + 1 < P) plan[p].end = in[p + 1];
        if (plan[p].in && (plan[p].in == plan[p].end || plan[p].in == plan[p].mid || plan[p].in == plan[p].pre ||
                           plan[p].in == plan[p].end2)) {   // (in null: a start from zero reads nothing)
            h->err = "internal: a face pass writes its own input";
            return PAMG_ERR_STATE;
        }
    }
    return PAMG_OK;
}

int face_pp_emit(pamg_handle *h, int l, const PPPass &q) {
    Level &L = h->lv[l];
    const int kid = (l == 1) ? PAMG_K_SMOOTH_L1 : PAMG_K_SMOOTH;
    // iterate and RHS in, the outputs and the residual out (the halo gathers of the neighbours' boundary
    // sub-elements are overhead, not counted)
    // (a start from zero reads no iterate; the folded interpolation reads the coarse level's, 6 B per sub-element)
    const double by = (24.0 * (q.in != nullptr) + 24.0 + (q.interp ? 6.0 : 0.0) + (q.rhsc ? 6.0 : 0.0) +
                       24.0 * ((q.pre != nullptr) + (q.mid != nullptr) + (q.end != nullptr) + (q.end2 != nullptr) +
                               (q.res != 0 && !q.res_drop))) * (double)L.N + 168.0 * h->U;
    if (q.res) h->rhsn_valid = false;
    Span sp(h, kid, by);
    PPCoarse pc;
    pc.coarse = (q.interp || q.rhsc) ? &h->lv[l + 1] : nullptr;
    pc.rhsc = q.rhsc;
    pc.res_store = !q.res_drop;
    pc.interp = q.interp;
    HIPCHK(h, launch_face_pp(h->stream, L, q.K, q.in, q.pre, q.mid, q.end, h->p.solver == 3, l == 1, 1 / h->p.dt, q.res,
                             q.end2, pc.coarse ? &pc : nullptr));
    return PAMG_OK;
}

// the coarsest level's two smoother calls of a cycle that is not the call's last as ONE call: the restriction
// leg's (:331, ns sweeps, the last dead: tnew := sweep ns - 1) and the coarse solve's (:344-359, ns n_coarse
// sweeps from tnew, the last dead). Between them the cycle computes only the coarsest residual (:338), which
// such a cycle skips (face_pp_level), and the second call's leg copy tnew_nonlin := tnew (:348) continues from
// the first call's tnew: one call of (ns - 1) + (ns n_coarse - 1) executed sweeps and a dead last one, whose
// halo words at the seam are the ones the first call's last executed sweep published -- the words of that tnew,
// as the second call's refresh would write them. (The two calls run in a call's last cycle, whose residual is
// state; the merged form is bitwise them: tests/test_face_operator.py, oracle parity.)
bool face_coarse_merged(pamg_handle *h, bool last) {
    return !last && h->p.n_smooth >= 1 && h->p.n_coarse >= 1;
}

// :336 for level l >= 2 of the face cycle: the restriction of level l's previous residual into level l+1's RHS -- the
// buffer a fold made in the previous cycle's pass (swapped in), else the restrictor
int face_restrict_prev(pamg_handle *h, int l) {
    if (h->pp_folded[l]) {
        std::swap(h->lv[l + 1].RHS, h->lv[l + 1].RHSN_alt);
        h->pp_folded[l] = false;
        return PAMG_OK;
    }
    return restrict_(h, l);
}

// level l's part of cycle c of the fused face cycle (levels l .. L): the coarsest level's calls; a level
// below it as a two-sweep stream (its restrictor before the launch that writes its new residual, then the
// next level), or as its two calls around the next level (vcycle_face_fused's order)
int face_pp_level(pamg_handle *h, int l, bool last) {
    const int L = h->p.multi_levels, ns = h->p.n_smooth;
    const double rdt = 1 / h->p.dt;
    if (l == L) {
        if (face_coarse_merged(h, last)) return face_call(h, L, true, ns + ns * h->p.n_coarse - 1, true);
        CHK(face_call(h, l, true, ns, true));   // :331 via :351
        Level &V = h->lv[l];
        h->rhsn_valid = false;
        // the coarsest level's get_residual (:338): nothing restricts or reads it (restrictor(L) is empty,
        // splitting.F90:18), and the next cycle rewrites it -- only the call's last cycle's is state
        if (last) {
            Span sp(h, PAMG_K_RESIDUAL, 72.0 * (double)V.N + 168.0 * h->U);
            HIPCHK(h, launch_face_residual(h->stream, V, h->tov, false, l == 1, rdt, h->slots));
        }
        return face_call(h, L, true, ns * h->p.n_coarse, !last);   // :344-359
    }
    if (!face_pp_ok(h, l) || 2 * (ns - 1) + (last ? 1 : 0) < 3) {   // (one pass could not rotate its buffers)
        CHK(face_call(h, l, true, ns, true));
        CHK(face_restrict_prev(h, l));
        CHK(face_pp_level(h, l + 1, last));
        return face_call(h, l, true, ns, !last, true);
    }
    h->tnn_level = l;
    h->overlap_static_l1 = false;
    std::vector<PPPass> plan;
    CHK(face_pp_plan(h, l, 2 * (ns - 1) + (last ? 1 : 0), h->lv[l].T, {ns - 1}, last ? 1 : 2, plan));
    // the restrictor folded (vcycle_face_pp's level-1 fold, one level down): the pass that computes this cycle's
    // residual restricts it into level l+1's RHSN_alt and, but in the call's last cycle, does not store it (only
    // the restrictor reads it); the next cycle swaps that buffer in where it would restrict
    const bool fold = h->pp_fold && h->lv[l + 1].RHSN_alt;
    bool restricted = false;
    for (const PPPass &q : plan) {
        if (q.res && !restricted) { CHK(face_restrict_prev(h, l)); restricted = true; }   // :336, the previous residual
        PPPass qf = q;
        if (q.res && fold && !last) {
            qf.rhsc = h->lv[l + 1].RHSN_alt;
            qf.res_drop = true;
        }
        CHK(face_pp_emit(h, l, qf));
        if (qf.rhsc) h->pp_folded[l] = true;
    }
    if (!restricted) CHK(face_restrict_prev(h, l));
    return face_pp_level(h, l + 1, last);
}

int vcycle_face_pp(pamg_handle *h, int n) {
    const int ns = h->p.n_smooth;
    if (n <= 0) return PAMG_OK;
    if (!face_pp_ok(h, 1)) {   // level 1 as its two calls per cycle, a coarser level as a stream
        for (int c = 0; c < n; ++c) CHK(face_pp_level(h, 1, c + 1 == n));
        h->tnn_level = 1;
        return face_chain_check(h);
    }
    // level 1: one stream over the call's cycles, get_residual after each cycle's restriction leg
    const int per = 2 * (ns - 1);
    std::vector<int> res_at;
    for (int c = 0; c < n; ++c) res_at.push_back(ns - 1 + per * c);
    std::vector<PPPass> plan;
    CHK(face_pp_plan(h, 1, per * n + 1, h->lv[1].T, res_at, 1, plan));
    h->overlap_static_l1 = false;
    // the restrictor folded into the pass that computes the residual (PAMG_FACE_RR=0: its own launch). The cycle
    // restricts the PREVIOUS cycle's residual (:336 before :338), so the pass that computes cycle c's residual
    // restricts it into level 2's second RHS buffer (RHSN_alt, unused by the face cycle) and cycle c + 1 swaps the
    // two instead of launching the restrictor; that residual is then not stored either (only the restrictor reads
    // it) -- except the call's last cycle's, which is the state, and which the next call's first cycle restricts
    const char *rr_env = getenv("PAMG_FACE_RR");
    Level &L2 = h->lv[2];
    const bool rf = !(rr_env && atoi(rr_env) == 0) && h->p.multi_levels >= 2 && L2.RHSN_alt;
    // levels 2 .. L: each RHS's own buffer (the folds swap RHS and RHSN_alt). An error return inside the loop leaves
    // the buffers as it found them (the state is invalid after an error, but RHS and RHSN_alt stay the handle's own
    // two buffers in their roles); the coarse levels' folds are off outside this call
    const int Lc = h->p.multi_levels;
    double *rhs_home[kMaxLevels + 1] = {};
    for (int l = 2; l <= Lc; ++l) rhs_home[l] = h->lv[l].RHS;
    struct Home {
        pamg_handle *h; int Lc; double *const *home;
        ~Home() {
            for (int l = 2; l <= Lc; ++l)
                if (h->lv[l].RHS != home[l]) std::swap(h->lv[l].RHS, h->lv[l].RHSN_alt);
            h->pp_fold = false;
            for (bool &f : h->pp_folded) f = false;
        }
    } home_guard{h, Lc, rhs_home};
    h->pp_fold = rf;
    size_t p = 0;
    for (int c = 0; c < n; ++c) {
        h->tnn_level = 1;
        if (c == 0 || !rf) CHK(restrict_(h, 1));   // :336 -- level 1's residual of the previous cycle, before this cycle's is written
        else std::swap(L2.RHS, L2.RHSN_alt);       // the restriction of it, made by the pass that computed it
        const size_t pr = (size_t)res_at[c] / 2;   // the pass that writes this cycle's residual
        for (; p <= pr; ++p) {
            PPPass q = plan[p];
            if (p == pr && rf && c + 1 < n) {
                q.rhsc = L2.RHSN_alt;
                q.res_drop = true;
            }
            CHK(face_pp_emit(h, 1, q));
        }
        CHK(face_pp_level(h, 2, c + 1 == n));
    }
    for (; p < plan.size(); ++p) CHK(face_pp_emit(h, 1, plan[p]));
    for (int l = 2; l <= Lc; ++l) {   // each RHS back in its own buffer
        Level &V = h->lv[l];
        if (V.RHS == rhs_home[l]) continue;
        HIPCHK(h, hipMemcpyAsync(V.RHSN_alt, V.RHS, 3 * (size_t)V.pitch * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        std::swap(V.RHS, V.RHSN_alt);
    }
    // the halo the per-step sequence leaves: level 1's last smoother call's words, from its tnew (:555)
    HIPCHK(h, launch_face_words(h->stream, h->lv[1], h->U, h->tov, h->tovo));
    h->tnn_level = 1;
    return face_chain_check(h);
}

// ---- op = 1 on a partition: the coarsest level agglomerated ----------------------------
// On a partition the coarsest level's smoother calls -- 62 of the cycle's 74 sweeps at the bench shape, each
// reading the halo words the neighbours' previous sweep wrote -- would be one launch and one exchange per sweep.
// The level is small (12.6 MB per field for all of untitled8192 at n_split 5) and, in the reference's cycle,
// nothing finer reads it back within a call (the prolongator's output is overwritten, SURVEY.md A3 iv); in the
// corrected cycle only its result is read. So every rank gathers the ranks' blocks of the level's RHS (the
// restriction of their own level-2 residuals, splitting.F90:10-32) into a replica of the WHOLE level (h->agg,
// single domain, renumbered rank block by rank block) and runs there the single-domain coarsest calls
// (transport_tri_semi.F90:331 via :351, :338, :344-359): the persistent chain, its halo words handed over inside
// the launch. The replicas stay identical on every rank (the same inputs through the same kernels), and a rank
// copies its own block of the result back into its level L. The replica's tnew carries over from call to call as
// the level's tnew does (it is never reset, A3 v); it is gathered from the ranks once at the start of each call,
// so a partition's level L written between calls by anything else (pamg_set_state, per-step calls) is picked up.
// Bitwise the single domain (tests/test_face_operator.py). PAMG_FACE_AGG=0 at upload keeps the per-sweep form.

// the local-group transport: every peer's block of a 3-plane field pulled from its handle, behind its event
int gather_local(pamg_handle *h, const double *local, int64_t lpitch, double *rep, int64_t rpitch, int nsub,
                 hipStream_t st) {
    Comm &C = *h->comm;
    LocalGroup &G = *C.local;
    const int me = h->rank, n = G.n;
    std::vector<LocalGroup::Post> got(n);
    auto wait_posts = [&](std::vector<LocalGroup::Post> &box, const char *what) -> int {
        std::unique_lock<std::mutex> lk(G.mu);
        for (int peer = 0; peer < n; ++peer) {
            if (peer == me) continue;
            const long want = C.seq[peer] + 1;
            LocalGroup::Post &b = box[(size_t)peer * n + me];
            if (!G.cv.wait_for(lk, std::chrono::seconds(local_timeout_s()), [&] { return b.seq >= want; })) {
                h->err = "local coarse gather: rank " + std::to_string(me) + " timed out waiting for rank " +
                         std::to_string(peer) + "'s " + what;
                return PAMG_ERR_COMM;
            }
            if (b.seq != want) { h->err = "local coarse gather: sequence mismatch"; return PAMG_ERR_COMM; }
            got[peer] = b;
        }
        return PAMG_OK;
    };
    HIPCHK(h, hipEventRecord(C.ev_ready, st));
    {
        std::lock_guard<std::mutex> lk(G.mu);
        for (int peer = 0; peer < n; ++peer)
            if (peer != me) G.ready[(size_t)me * n + peer] = {C.seq[peer] + 1, local, C.ev_ready, lpitch};
    }
    G.cv.notify_all();
    CHK(wait_posts(G.ready, "coarse block"));
    for (int peer = 0; peer < n; ++peer) {
        if (peer == me) continue;
        const size_t cnt = (size_t)(h->agg_off[peer + 1] - h->agg_off[peer]) * nsub;
        HIPCHK(h, hipStreamWaitEvent(st, got[peer].ev, 0));
        if (cnt)
            HIPCHK(h, hipMemcpy2DAsync(rep + (size_t)h->agg_off[peer] * nsub, rpitch * sizeof(double), got[peer].ptr,
                                       got[peer].pitch * sizeof(double), cnt * sizeof(double), 3,
                                       hipMemcpyDeviceToDevice, st));
    }
    // this rank's reads are issued; its own block may change once every peer's are
    HIPCHK(h, hipEventRecord(C.ev_done, st));
    {
        std::lock_guard<std::mutex> lk(G.mu);
        for (int peer = 0; peer < n; ++peer)
            if (peer != me) G.done[(size_t)me * n + peer] = {C.seq[peer] + 1, nullptr, C.ev_done, 0};
    }
    G.cv.notify_all();
    CHK(wait_posts(G.done, "read completion"));
    for (int peer = 0; peer < n; ++peer) {
        if (peer == me) continue;
        HIPCHK(h, hipStreamWaitEvent(st, got[peer].ev, 0));
        C.seq[peer] += 1;
    }
    return PAMG_OK;
}

// RCCL: one grouped send / recv per peer and plane (an allgatherv of the blocks); a self-peer communicator
// (pamg_comm_init_self) sends its whole level to itself through RCCL, so the transport runs on one GPU
int gather_rccl(pamg_handle *h, const double *local, int64_t lpitch, double *rep, int64_t rpitch, int nsub,
                hipStream_t st) {
    const bool self_peer = !h->vpart.empty();
    const size_t mine = (size_t)h->U * nsub;
    NCCLCHK(h, ncclGroupStart());
    for (int r = 0; r < h->nranks; ++r) {
        if (r == h->rank && !self_peer) continue;   // (copied on the device)
        const size_t cnt = (size_t)(h->agg_off[r + 1] - h->agg_off[r]) * nsub;
        for (int c = 0; c < 3; ++c) {
            if (mine) NCCLQ(h, ncclSend(local + c * lpitch, mine, ncclDouble, r, h->comm->nccl, st));
            if (cnt)
                NCCLQ(h, ncclRecv(rep + c * rpitch + (size_t)h->agg_off[r] * nsub, cnt, ncclDouble, r, h->comm->nccl, st));
        }
    }
    return nccl_group_end(h);
}

// level L's field `local` of every rank into the replica's `rep`
int agg_gather(pamg_handle *h, const double *local, double *rep) {
    const int L = h->p.multi_levels;
    const Level &V = h->lv[L], &R = h->agg->lv[L];
    Span sp(h, PAMG_K_COARSE_GATHER, 24.0 * (double)R.N);   // the whole level arrives (this rank's block by copy)
    const bool self_peer = !h->vpart.empty();
    if (!self_peer && h->U)
        HIPCHK(h, hipMemcpy2DAsync(rep + (size_t)h->agg_off[h->rank] * V.nsub, R.pitch * sizeof(double), local,
                                   V.pitch * sizeof(double), (size_t)h->U * V.nsub * sizeof(double), 3,
                                   hipMemcpyDeviceToDevice, h->stream));
    if (h->comm && h->comm->nccl) return gather_rccl(h, local, V.pitch, rep, R.pitch, V.nsub, h->stream);
    if (h->comm && h->comm->local) return gather_local(h, local, V.pitch, rep, R.pitch, V.nsub, h->stream);
    return PAMG_OK;   // a detached partition (timing probes): its own block only
}

// this rank's block of the replica's level-L fields back into its own level L
int agg_copy_back(pamg_handle *h, bool res) {
    const int L = h->p.multi_levels;
    Level &V = h->lv[L];
    const Level &R = h->agg->lv[L];
    if (!h->U) return PAMG_OK;
    const size_t off = (size_t)h->agg_off[h->vpart.empty() ? h->rank : 0] * V.nsub;
    for (int f = 0; f < 3; ++f) {
        if (f == 2 && !res) continue;
        double *dst = f == 0 ? V.T : f == 1 ? V.TNN : V.RES;
        const double *src = f == 0 ? R.T : f == 1 ? R.TNN : R.RES;
        HIPCHK(h, hipMemcpy2DAsync(dst, V.pitch * sizeof(double), src + off, R.pitch * sizeof(double),
                                   (size_t)h->U * V.nsub * sizeof(double), 3, hipMemcpyDeviceToDevice, h->stream));
    }
    return PAMG_OK;
}

// the reference cycle's coarsest-level work of cycle c (vcycle_face_fused: the restriction-leg call, the
// residual in the call's last cycle, the coarse solve -- or their merged call) on the replica
int agg_coarse_cycle(pamg_handle *h, bool first, bool last) {
    const int L = h->p.multi_levels;
    pamg_handle *r = h->agg;
    if (first) CHK(agg_gather(h, h->lv[L].T, r->lv[L].T));
    CHK(agg_gather(h, h->lv[L].RHS, r->lv[L].RHS));
    CHK(face_pp_level(r, L, last));
    return last ? agg_copy_back(h, true) : PAMG_OK;
}

// one smoother call of the corrected cycle on level l < L: tnew := the result of n_smooth sweeps from tnew;
// streaming levels only (face_pp_ok): from_zero -- from a zero iterate (the cycle's memset of a coarse level
// folded: the first pass reads no iterate), interp -- from tnew plus the prolonged coarse correction (the
// cycle's interp_add folded into the first pass, which adds it to every value it loads: bitwise the
// correction stored and read back; the corrected iterate itself is overwritten unread by the call's result)
int face_corr_call(pamg_handle *h, int l, bool last, bool from_zero = false, bool interp = false) {
    const int ns = h->p.n_smooth;
    if (!face_pp_ok(h, l)) {
        if (from_zero || interp) { h->err = "internal: a folded face call on a level that does not stream"; return PAMG_ERR_STATE; }
        CHK(smooth_to_tnew(h, l, ns));
        return PAMG_OK;
    }
    h->tnn_level = l;
    h->overlap_static_l1 = false;
    std::vector<PPPass> plan;
    CHK(face_pp_plan(h, l, ns, from_zero ? nullptr : h->lv[l].T, {}, last ? 3 : 2, plan));
    plan[0].interp = interp;
    for (const PPPass &q : plan) CHK(face_pp_emit(h, l, q));
    return PAMG_OK;
}

// the corrected cycle's get_residual and restrictor of a level l < L (:336-338) as one sweep-less k_face_pp pass
// (res 3): the residual RHS - A tnew from the neighbours' iterate itself, restricted straight into RHS_{l+1}
// (k_restrict_tile's arithmetic). The residual is stored only where the state keeps it: level 1's is rewritten
// by the fine residual after the cycle (the call's last cycle); a coarser level's is kept from the call's last
// cycle. The halo words the per-step residual refreshes first are rewritten, unread, by that same fine residual
// (every coarser level's words are a subset of level 1's slots).
int face_res_restrict(pamg_handle *h, int l, bool last) {
    Level &L = h->lv[l];
    h->rhsn_valid = false;
    h->overlap_static_l1 = false;
    const bool store = l > 1 && last;
    Span sp(h, PAMG_K_RESIDUAL, (48.0 + (store ? 24.0 : 0.0)) * (double)L.N + 24.0 * (double)h->lv[l + 1].N + 168.0 * h->U);
    PPCoarse pc;
    pc.coarse = &h->lv[l + 1];
    pc.rhsc = h->lv[l + 1].RHS;
    pc.res_store = store;
    HIPCHK(h, launch_face_pp(h->stream, L, 1, L.T, nullptr, nullptr, nullptr, h->p.solver == 3, l == 1, 1 / h->p.dt, 3,
                             nullptr, &pc));
    return PAMG_OK;
}

}  // namespace

namespace pamg {
namespace host {

// the give-up word of the chain's bounded spins: a call that hit it failed, and
// the state it left was computed from halo words that had not all arrived -- the handle's fields are
// invalid after the error (set them again, or start a new time step from a known tnew). Checked only
// when such a launch ran since the last check (the other op = 1 calls stay asynchronous); the word is
// cleared once reported, so the next call on the handle runs again.
int face_chain_check(pamg_handle *h) {
    CHK(face_gates_drain(h));
    if (h->agg) {
        const int rc = face_chain_check(h->agg);
        if (rc != PAMG_OK) { h->err = h->agg->err; return rc; }
    }
    if (!h->chain_tmo || !h->chain_pending) return PAMG_OK;
    h->chain_pending = false;
    unsigned v = 0;
    HIPCHK(h, hipMemcpyAsync(&v, h->chain_tmo, sizeof v, hipMemcpyDeviceToHost, h->stream));
    CHK(sync_stream(h, h->stream));
    if (v) {
        HIPCHK(h, hipMemsetAsync(h->chain_tmo, 0, sizeof v, h->stream));
        h->err = "face chain: a workgroup gave up waiting for its neighbours' halo words (the state is invalid)";
        return PAMG_ERR_HIP;
    }
    return PAMG_OK;
}

// a sweep as one launch on LDS tiles (k_face_tile / k_face_sweep) instead of the two colour
// launches (the per-colour kernels remain for the level shapes the tiles do not cover)
// ... and the whole smoother call with the halo words handed from sweep to sweep on the device
// (face_call; on a partition the words a launch writes for the next sweep -- the remote ones into the send
// buffer -- are exchanged before that sweep, into the snapshot buffer it reads)
bool face_tiles_ok(pamg_handle *h, int l) { return h->p.op == 1 && face_sweep_fusable(h->lv[l]); }

// read back the gated chain launches in stream order: each one's report arrives once it has run (its
// workgroups all resident: it opened its gate itself) or given up (the stream waits at its gate: the call
// runs here with one launch per sweep on stream_fb, from the input and snapshot the aborted launch left
// untouched, and then opens the gate). Every host wait on the handle's stream drains them first.
int face_gates_drain(pamg_handle *h) {
    if (h->agg) {   // the coarsest level's replica runs its chains on this handle's stream
        const int rc = face_gates_drain(h->agg);
        if (rc != PAMG_OK) { h->err = h->agg->err; return rc; }
    }
    while (!h->gates.empty()) {
        const pamg_handle::GatePending g = h->gates.front();
        h->gates.erase(h->gates.begin());
        volatile unsigned long long *st = h->gate_stat + (g.seq & (kGateRing - 1));
        const auto t0 = std::chrono::steady_clock::now();
        unsigned long long v = 0;
        for (unsigned i = 0;; ++i) {
            v = *st;
            if ((v >> 1) == g.seq) break;
            if ((i & 4095) != 4095) continue;
            const hipError_t e = hipStreamQuery(h->stream);
            if (e != hipSuccess && e != hipErrorNotReady) {
                h->gates.clear();
                HIPCHK(h, e);
            }
            if ((e == hipSuccess && (*st >> 1) != g.seq) ||
                std::chrono::steady_clock::now() - t0 > std::chrono::seconds(600)) {
                h->gates.clear();
                h->err = "face chain: a gated launch never reported (the state is invalid)";
                return PAMG_ERR_HIP;
            }
        }
        if (!(v & 1)) continue;
        Level &L = h->lv[g.l];
        double *const keep[3] = {L.T, L.TNN, L.RHS};
        const hipStream_t main = h->stream;
        L.T = g.T;
        L.TNN = g.TNN;
        L.RHS = g.RHS;
        h->stream = h->stream_fb;
        int rc = face_call_sweeps(h, g.l, g.sweeps, g.run, g.dead_last, g.src_is_T, g.both, false);
        if (rc == PAMG_OK && hipMemsetAsync(h->chain_tmo + 3, 0, sizeof(unsigned), h->stream) != hipSuccess) rc = PAMG_ERR_HIP;
        if (rc == PAMG_OK && hipStreamWriteValue64(h->stream, h->gate, g.want, 0) != hipSuccess) rc = PAMG_ERR_HIP;
        h->stream = main;
        L.T = keep[0];
        L.TNN = keep[1];
        L.RHS = keep[2];
        if (rc != PAMG_OK) {
            h->gates.clear();
            if (h->err.empty()) h->err = "face chain: the gated fallback failed to launch";
            return rc;
        }
        (h->tparent ? h->tparent : h)->timing.seq[PAMG_K_FACE_FALLBACK] += 1;
    }
    return PAMG_OK;
}

// res: also get_residual of level l (A tnew - RHS with the halo refreshed from tnew, :725-873) before
// the call changes tnew -- computed by the call's first tile sweep from the iterate and snapshot it
// loads anyway (the residual's own launch read tnew and RHS again), or by its own launch when the call
// runs another form
// both (not with dead_last): the call's result also into tnew -- the corrected cycle's tnew := tnew_nonlin after
// the call (smooth_to_tnew), made by the chain's final stores instead of a copy launch
int face_call(pamg_handle *h, int l, bool src_is_T, int sweeps, bool dead_last, bool res, bool both) {
    Level &L = h->lv[l];
    h->tnn_level = l;
    h->overlap_static_l1 = false;
    const double rdt = 1 / h->p.dt;
    const int kid = (l == 1) ? PAMG_K_SMOOTH_L1 : PAMG_K_SMOOTH;
    // src_is_T (the leg copy tnew_nonlin := tnew, :327 / :348 / :367): no copy launch. The call's first
    // sweep reads its iterate from tnew, which already holds what :550 would copy into it, and writes
    // tnew_nonlin for every sub-element; the halo refresh then only writes the words (it reads just the
    // sub-elements that have words). A dead-last call of one executed sweep (store 2) leaves
    // tnew_nonlin unwritten: the cycle overwrites it unread, as it does the dead sweep's.
    if (!h->tov_b) CHK(dev_alloc(h, &h->tov_b, (size_t)h->slots * 3 * std::max(h->U, 1)));
    double *buf[2] = {h->tov, h->tov_b};
    const int run = dead_last ? sweeps - 1 : sweeps;   // the sweeps that are executed
    // the residual in the first tile sweep: src_is_T (its iterate is tnew) and the tile loop below
    const bool res_in_sweep = res && src_is_T && run >= 1 && face_tile_shape(L) && !(run >= 2 && face_chain_ok(h, l));
    if (res && !res_in_sweep) CHK(face_residual(h, l, false));
    if (run <= 0) {   // a call of one dead sweep: tnew := tnew_nonlin and its :555 words
        if (src_is_T && !dead_last) HIPCHK(h, launch_copy(h->stream, L.T, L.TNN, 3 * L.pitch));
        if (sweeps > 0) {
            if (src_is_T) HIPCHK(h, launch_face_words(h->stream, L, h->U, h->tov, h->tovo));
            else HIPCHK(h, launch_face_halo(h->stream, L, h->tov, h->tovo, true));
            CHK(halo(h, l));
        }
        return PAMG_OK;
    }
    if (src_is_T) HIPCHK(h, launch_face_words(h->stream, L, h->U, buf[(sweeps - 1) & 1], h->tovo));   // :555
    else HIPCHK(h, launch_face_halo(h->stream, L, buf[(sweeps - 1) & 1], h->tovo, true));   // :550, :555
    CHK(halo(h, l, buf[(sweeps - 1) & 1]));   // a partition: the remote words into the same snapshot
    if (run >= 2 && face_chain_ok(h, l)) {   // the whole call in one launch
        CHK(face_chain_setup(h, l));
        if ((unsigned long long)L.chain_epoch + run + 2 >= 0xffffffffull) {   // the epoch would wrap: start over
            HIPCHK(h, hipMemsetAsync(L.chain_flags, 0, L.chain_flag_bytes, h->stream));
            L.chain_epoch = 0;
        }
        const unsigned f0 = L.chain_epoch;
        L.chain_epoch += (unsigned)run + 1;
        ChainGate G;
        CHK(face_gate_setup(h));
        if (h->gates.size() >= kGateRing / 2) CHK(face_gates_drain(h));   // (the status ring's reuse)
        G.gate = h->gate;
        G.stat = h->gate_stat;
        G.seq = h->gate_seq;
        {
            // the state crosses HBM once per call: tnew_nonlin and RHS in, tnew (+ tnew_nonlin) out
            Span sp(h, kid, (dead_last ? 72.0 : 96.0) * (double)L.N + 168.0 * h->U);
            h->chain_pending = true;
            HIPCHK(h, launch_face_chain(h->stream, L, h->U, h->cus, h->tov, h->tov_b, h->tovo, L.chain_flags,
                                        L.chain_nb_off, L.chain_nb_list, h->chain_tmo, run, sweeps,
                                        dead_last ? 2 : both ? 3 : 1,
                                        h->p.solver == 3, l == 1, rdt, h->p.omega, h->slots, src_is_T, f0, 1, G));
        }
        // fail safe: a launch whose workgroups were not all resident (a CU-masked stream, another stream's or
        // process's kernels on the CUs) aborted before touching anything -- the call runs with one launch per
        // sweep, from the same input and halo snapshot: the stream waits for the launch's report at its gate and
        // the host runs the fallback when it reads the report back (face_gates_drain, at the latest when the API
        // call ends). (Round 5's first form, the host waiting for every launch, cost 2.3 % more; removed.)
        h->gate_seq += 1;
        h->gate_base += 1;
        HIPCHK(h, hipStreamWaitValue64(h->stream, h->gate, h->gate_base, hipStreamWaitValueGte));
        h->gates.push_back({G.seq, h->gate_base, l, sweeps, run, dead_last, src_is_T, both, L.T, L.TNN, L.RHS});
        return PAMG_OK;
    }
    return face_call_sweeps(h, l, sweeps, run, dead_last, src_is_T, both, res_in_sweep);
}

// face-coupled operator: residual A tnew - RHS (neg: RHS - A tnew) with the halo refreshed from tnew
int face_residual(pamg_handle *h, int l, bool neg) {
    Level &L = h->lv[l];
    h->rhsn_valid = false;
    h->overlap_static_l1 = false;
    HIPCHK(h, launch_face_words(h->stream, L, h->U, h->tov, h->tovo));
    CHK(halo(h, l));
    // tnew, RHS in, residual out (the neighbours' values are the same tnew, gathered from cache)
    Span sp(h, PAMG_K_RESIDUAL, 72.0 * (double)L.N + 168.0 * h->U);
    HIPCHK(h, launch_face_residual(h->stream, L, h->tov, neg, l == 1, 1 / h->p.dt, h->slots));
    return PAMG_OK;
}

// The face-coupled operator's V-cycle (op = 1, cycle = 0) on a single domain, as the per-step
// sequence above with its dead work dropped: a smoother call's last sweep only makes a
// tnew_nonlin that the cycle overwrites before any read (:367 after the restriction leg, :348 at the
// coarsest level, the next cycle's :327 after the prolongation leg), so it runs only in the call's
// last cycle, where it is observable; the sweep before it leaves tnew and the dead sweep's halo words
// (face_call), which are also what get_residual's refresh from tnew (:555 via update_overlaps) would
// write, so the residual reads them as they are; the prolongator's output is overwritten by the
// smoother's first statement (:550, SURVEY.md A3 iv) and is not computed. The state after a call --
// every field of every level, t_overlap, t_overlap_old -- is bitwise the per-step sequence's
// (tests/test_face_operator.py).
bool face_cycle_fusable(pamg_handle *h) {
    if (!(h->p.fused && h->p.op == 1 && h->p.cycle == 0 && h->p.coarse_solver == 0)) return false;
    for (int l = 1; l <= h->p.multi_levels; ++l)
        if (!face_tiles_ok(h, l)) return false;
    return true;
}

// the corrected cycle's coarse solve (vcycle_corrected: tnew := 0, n_smooth n_coarse sweeps, tnew := the
// result) on the replica; its result is read by the interpolation into level L - 1
int agg_coarse_corrected(pamg_handle *h) {
    const int L = h->p.multi_levels, ns = h->p.n_smooth;
    pamg_handle *r = h->agg;
    Level &C = r->lv[L];
    CHK(agg_gather(h, h->lv[L].RHS, C.RHS));
    HIPCHK(h, hipMemsetAsync(C.T, 0, 3 * (size_t)C.pitch * sizeof(double), h->stream));   // from zero
    if (ns * h->p.n_coarse > 0 && face_tiles_ok(r, L)) CHK(face_call(r, L, true, ns * h->p.n_coarse, false, false, true));
    else CHK(smooth_to_tnew(r, L, ns * h->p.n_coarse));
    return agg_copy_back(h, false);
}

int vcycle_face_fused(pamg_handle *h, int n) {
    if (h->p.multi_levels >= 2 && h->p.n_smooth >= 2)
        for (int l = 1; l < h->p.multi_levels; ++l)
            if (face_pp_ok(h, l)) return vcycle_face_pp(h, n);
    const int L = h->p.multi_levels, ns = h->p.n_smooth;
    const double rdt = 1 / h->p.dt;
    for (int c = 0; c < n; ++c) {
        const bool last = c + 1 == n;
        for (int l = 1; l <= L; ++l) {   // :323-340
            if (l == L && h->agg) break;   // (the replica runs the coarsest level, below)
            if (l == L && face_coarse_merged(h, last)) break;   // (the call below runs both)
            CHK(face_call(h, l, true, ns, true));
            CHK(restrict_(h, l));
            if (l < L) continue;   // levels < L: get_residual rides on the prolongation-leg call below
            if (!last) continue;   // the coarsest level's: read by nothing, rewritten next cycle (face_pp_level)
            Level &V = h->lv[l];
            h->rhsn_valid = false;
            Span sp(h, PAMG_K_RESIDUAL, 72.0 * (double)V.N + 168.0 * h->U);   // tnew, RHS in, residual out
            HIPCHK(h, launch_face_residual(h->stream, V, h->tov, false, l == 1, rdt, h->slots));
        }
        if (h->agg) CHK(agg_coarse_cycle(h, c == 0, last));   // a partition: the agglomerated coarsest level
        else if (face_coarse_merged(h, last)) CHK(face_call(h, L, true, ns + ns * h->p.n_coarse - 1, true));
        else CHK(face_call(h, L, true, ns * h->p.n_coarse, !last));   // :344-359
        // :363-378; the residual of the restriction leg (:336) is due after the level's call there, and
        // nothing changes level l's tnew, RHS or halo words until this call starts: it computes it
        for (int l = L - 1; l >= 1; --l) CHK(face_call(h, l, true, ns, !last, true));
    }
    h->tnn_level = 1;
    return face_chain_check(h);
}

// The corrected cycle on the face-coupled operator (op = 1, cycle = 1) with the smoother calls of the levels
// below the coarsest as two-sweep passes (k_face_pp; single domain, face_pp_ok) instead of one launch per
// sweep and a copy: each call runs its n_smooth sweeps from tnew in passes whose last one stores the result
// as tnew (and, in the call's last cycle, as tnew_nonlin too -- inside the call tnew_nonlin is overwritten
// before any read); the coarsest level's calls stay one chain launch (face_call). The passes do not publish
// halo words between sweeps (they read the neighbours' iterate itself), and no operation of the cycle reads
// t_overlap but the residuals, each of which refreshes the words from its level's tnew first (face_residual)
// -- as does the per-step sequence's last operation, the fine residual after the cycle, which only the
// call's last cycle runs here (the next cycle's first residual rewrites it unread, and its words). Every
// sub-element's arithmetic is face_apply's: the state after the call is bitwise vcycle_corrected's
// (tests/test_face_operator.py). PAMG_FACE_CORR_PP=0 keeps the per-step sequence (A/B).
bool face_corrected_pp_ok(pamg_handle *h) {
    const char *ev = getenv("PAMG_FACE_CORR_PP");   // read per call: tests switch it within a process
    const bool off = ev && atoi(ev) == 0;
    if (off || !(h->p.op == 1 && h->p.cycle == 1 && h->p.fused && h->p.coarse_solver == 0 && h->p.n_smooth >= 3 &&
                 h->p.multi_levels >= 2))
        return false;
    for (int l = 1; l < h->p.multi_levels; ++l)
        if (face_pp_ok(h, l)) return true;
    return false;
}

int vcycle_corrected_face_pp(pamg_handle *h, int n) {
    const int L = h->p.multi_levels, ns = h->p.n_smooth;
    h->overlap_static_l1 = false;
    // PAMG_FACE_RR=0 (A/B): the residual and the restrictor as their own launches; PAMG_FACE_FOLD=0: a coarse
    // level's memset and the interpolation as their own launches
    const char *rr_env = getenv("PAMG_FACE_RR"), *fold_env = getenv("PAMG_FACE_FOLD");
    const bool rr = !(rr_env && atoi(rr_env) == 0), fold = !(fold_env && atoi(fold_env) == 0);
    for (int c = 0; c < n; ++c) {
        const bool last = c + 1 == n;
        for (int l = 1; l < L; ++l) {
            const bool fz = l > 1 && fold && face_pp_ok(h, l);
            if (l > 1 && !fz) HIPCHK(h, hipMemsetAsync(h->lv[l].T, 0, 3 * (size_t)h->lv[l].pitch * sizeof(double), h->stream));
            CHK(face_corr_call(h, l, last, fz));
            if (rr && face_pp_ok(h, l)) {
                CHK(face_res_restrict(h, l, last));
            } else {
                CHK(residual_corrected(h, l));
                CHK(restrict_(h, l));
            }
        }
        Level &C = h->lv[L];
        HIPCHK(h, hipMemsetAsync(C.T, 0, 3 * (size_t)C.pitch * sizeof(double), h->stream));   // from zero
        if (fold && ns * h->p.n_coarse > 0 && face_tiles_ok(h, L)) {
            CHK(face_call(h, L, true, ns * h->p.n_coarse, false, false, true));   // tnew := the result: the final stores
        } else {
            CHK(smooth_to_tnew(h, L, ns * h->p.n_coarse));
        }
        for (int l = L - 1; l >= 1; --l) {
            if (fold && face_pp_ok(h, l)) {
                CHK(face_corr_call(h, l, last, false, true));
                continue;
            }
            {
                Span sp(h, PAMG_K_PROLONG, 216.0 * (double)h->lv[l + 1].N);
                HIPCHK(h, launch_interp_add(h->stream, h->lv[l], h->lv[l + 1]));
            }
            CHK(face_corr_call(h, l, last));
        }
        if (last) CHK(residual_corrected(h, 1));   // the fine residual after the cycle
    }
    h->tnn_level = 1;
    return face_chain_check(h);
}

// the replica of the coarsest level for op = 1 on a partition (agg_coarse_cycle); PAMG_FACE_AGG=0 (read here, at
// upload): none -- the partition then runs its coarsest calls one launch per sweep, exchanging between sweeps
int agg_create(pamg_handle *h, int U, const double *X, const int *region, const int *neig, const int *fneig,
               const int *dir) {
    const char *e = getenv("PAMG_FACE_AGG");
    const int L = h->p.multi_levels;
    if (h->coarse_only || h->p.op != 1 || L < 2 || (h->nranks == 1 && h->vpart.empty()) || (e && atoi(e) == 0))
        return PAMG_OK;
    // only a level the persistent chain holds: that is what makes the whole level cost every rank no more than its
    // own part did (latency-bound sweeps); a larger coarsest level stays partitioned, one launch per sweep
    if (!face_chain_fits(1 << (2 * (h->p.n_split - L + 1)), U, device_cus(h))) return PAMG_OK;
    // the replica's numbering: rank 0's un_eles (ascending global id), then rank 1's, ... (a self-peer
    // communicator: one block, the global order)
    std::vector<int> order;
    order.reserve(U);
    h->agg_off.assign(1, 0);
    if (h->nranks == 1) {
        for (int g = 0; g < U; ++g) order.push_back(g);
        h->agg_off.push_back(U);
    } else {
        for (int r = 0; r < h->nranks; ++r) {
            for (int g = 0; g < U; ++g)
                if (h->owner[g] == r) order.push_back(g);
            h->agg_off.push_back((int)order.size());
        }
    }
    std::vector<int> pnew(U);
    for (int i = 0; i < U; ++i) pnew[order[i]] = i;
    std::vector<double> Xp(6 * (size_t)U);
    std::vector<int> regp(U), neigp(3 * (size_t)U), fneigp(3 * (size_t)U), dirp(3 * (size_t)U);
    for (int i = 0; i < U; ++i) {
        const int g = order[i];
        for (int c = 0; c < 6; ++c) Xp[6 * (size_t)i + c] = X[6 * (size_t)g + c];
        regp[i] = region[g];
        for (int f = 0; f < 3; ++f) {
            const int nb = neig[3 * (size_t)g + f];
            neigp[3 * (size_t)i + f] = nb >= 1 ? pnew[nb - 1] + 1 : nb;
            fneigp[3 * (size_t)i + f] = fneig[3 * (size_t)g + f];
            dirp[3 * (size_t)i + f] = dir[3 * (size_t)g + f];
        }
    }
    // the replica works on this handle's streams (its chains are ordered with the cycle) and creates none of its
    // own but the chain gates' fallback stream, on first use: a process then holds the four streams of a
    // single-domain handle, one per hardware queue (GPU_MAX_HW_QUEUES = 4), so the fallback never waits behind
    // the gate it opens
    auto *r = new pamg_handle;
    r->p = h->p;
    r->device = h->device;
    r->stream = h->stream;
    r->stream_comm = h->stream_comm;
    r->stream_c = h->stream_c;
    r->borrowed_stream = true;
    r->coarse_only = true;
    r->tparent = h;
    r->cus = h->cus;
    const int rc = pamg_upload_mesh(r, U, Xp.data(), regp.data(), neigp.data(), fneigp.data(), dirp.data());
    if (rc != PAMG_OK) {
        h->err = "coarse replica: " + r->err;
        (void)pamg_destroy(r);
        return rc;
    }
    h->agg = r;
    return PAMG_OK;
}

// ---- the face operator's convergence monitor (pamg_params.monitor = 1, op = 1) ----
// the monitor's image (t_overlap's size) and the send / receive words of its exchange, 3 per entry, sized for
// the largest level's plan; on the first check
int monitor_setup(pamg_handle *h) {
    if (h->mon_img) return PAMG_OK;
    size_t ns = 0, nr = 0;
    for (int l = 1; l <= h->p.multi_levels; ++l) {
        ns = std::max(ns, h->lv[l].halo.remote.size());
        nr = std::max(nr, h->lv[l].halo.recv_dst.size());
    }
    const size_t n = (size_t)h->slots * 3 * std::max(h->U, 1);
    double *img = nullptr, *snd = nullptr, *rcv = nullptr;
    if (dev_alloc(h, &img, n) != PAMG_OK || dev_alloc(h, &snd, 3 * ns) != PAMG_OK ||
        dev_alloc(h, &rcv, 3 * nr) != PAMG_OK) {
        dev_free(img); dev_free(snd); dev_free(rcv);
        return PAMG_ERR_HIP;
    }
    h->mon_img = img; h->mon_send = snd; h->mon_recv = rcv;
    HIPCHK(h, hipMemsetAsync(img, 0, n * sizeof(double), h->stream));
    return PAMG_OK;
}

// the monitor words of level l that face un_eles of other ranks: exchange_ring's exchange (3 words per entry) of
// the monitor's own send words into its own receive words on the handle's stream, unpacked into its image
int monitor_exchange(pamg_handle *h, int l) {
    Level &L = h->lv[l];
    const HaloPlan &P = L.halo;
    if (!h->comm || P.peers.empty()) return PAMG_OK;
    hipStream_t st = h->stream;
    if (h->comm->local) {
        CHK(exchange_local(h, l, h->mon_send, st, 3, h->mon_recv));
    } else {
        NCCLCHK(h, ncclGroupStart());
        for (size_t q = 0; q < P.peers.size(); ++q) {
            const int peer = P.peers[q];
            const size_t ns = (size_t)(P.send_peer_off[q + 1] - P.send_peer_off[q]);
            const size_t nr = (size_t)(P.recv_peer_off[q + 1] - P.recv_peer_off[q]);
            if (ns) NCCLQ(h, ncclSend(h->mon_send + 3 * (size_t)P.send_peer_off[q], 3 * ns, ncclDouble, peer,
                                      h->comm->nccl, st));
            if (nr) NCCLQ(h, ncclRecv(h->mon_recv + 3 * (size_t)P.recv_peer_off[q], 3 * nr, ncclDouble, peer,
                                      h->comm->nccl, st));
        }
        CHK(nccl_group_end(h));
    }
    HIPCHK(h, launch_halo_unpack3(st, L, h->mon_img, h->mon_recv));
    return PAMG_OK;
}

}  // namespace host
}  // namespace pamg
