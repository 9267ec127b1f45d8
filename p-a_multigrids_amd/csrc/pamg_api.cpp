// C-ABI of libpamg: handle, setup, state transfer and the hot-path entry points
// (one per reference call site); the code behind them is in pamg_comm.cpp,
// pamg_face_host.cpp, pamg_cycle.cpp and pamg_norm_host.cpp (pamg_host.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "pamg_host.h"

using namespace pamg;
using namespace pamg::host;

namespace {

void free_levels(pamg_handle *h) {
    for (int l = 1; l <= kMaxLevels; ++l) {
        Level &L = h->lv[l];
        dev_free(L.ERR);
        dev_free(L.T); dev_free(L.stc); dev_free(L.Ainv); dev_free(L.subinfo); dev_free(L.d_pos); dev_free(L.blocks);
        dev_free(L.fnb); dev_free(L.fface); dev_free(L.fsx); dev_free(L.cpos); dev_free(L.gtab); dev_free(L.cnb); dev_free(L.gpat);
        dev_free(L.chain_nb_off); dev_free(L.chain_nb_list); dev_free(L.chain_flags);
        dev_free(L.halo.d_local); dev_free(L.halo.d_bc); dev_free(L.halo.d_remote); dev_free(L.halo.d_recv_dst);
        dev_free(L.halo.d_send); dev_free(L.halo.d_send_b); dev_free(L.halo.d_recv);
        dev_free(L.halo.d_ring); dev_free(L.halo.d_recv3);
        dev_free(L.halo.d_hface); dev_free(L.halo.d_hsub); dev_free(L.halo.d_bcv); dev_free(L.halo.d_bpos);
        dev_free(L.halo.d_surf); dev_free(L.halo.d_told_halo);
        L = Level();
    }
    dev_free(h->geo1); dev_free(h->tov); dev_free(h->tovo); dev_free(h->tov_b);
    h->geo1 = h->tov = h->tovo = h->tov_b = nullptr;
    dev_free(h->xe_map);
    h->xe_map = nullptr;
    h->xe_nremote = -1;
    dev_free(h->mon_img); dev_free(h->mon_send); dev_free(h->mon_recv);
    h->mon_img = h->mon_send = h->mon_recv = nullptr;
    h->mesh_ready = false;
}

}  // namespace

extern "C" {

int pamg_version(void) { return 100; }

void pamg_default_params(pamg_params *p) {
    std::memset(p, 0, sizeof *p);
    p->n_split = 1;          // :118
    p->multi_levels = 1;     // main.F90:46-47
    p->n_smooth = 4;
    p->n_coarse = 15;        // :351
    p->solver = 3;
    p->device = 0;
    p->dt = 1. * 0.0000125;  // CFL*dx, :133
    p->k = 1.;               // :136
    p->omega = 0.8;          // :140
    p->theta = 1.;           // :117
    p->halo_mode = 0;
    p->fused = 3;
}

int pamg_create(const pamg_params *p, pamg_handle **out) {
    if (!p || !out) return PAMG_ERR_ARG;
    *out = nullptr;
    if (p->multi_levels < 1 || p->multi_levels > p->n_split || p->n_split > kMaxLevels || p->n_split < 1 ||
        p->n_smooth < 1 || p->n_coarse < 0 || (p->solver < 1 || p->solver > 3) || !(p->dt > 0) ||
        p->theta != 1.0 || (p->halo_mode != 0 && p->halo_mode != 1) ||
        (p->coarse_solver != 0 && p->coarse_solver != 1) || p->fused < 0 || p->fused > 3 ||
        (p->arith != 0 && p->arith != 1) || (p->halo_exchange != 0 && p->halo_exchange != 1) ||
        (p->cycle != 0 && p->cycle != 1) || (p->cycle == 1 && p->solver == 2) || (p->op != 0 && p->op != 1) ||
        (p->op == 1 && (p->solver == 2 || p->coarse_solver == 1)) || (p->monitor != 0 && p->monitor != 1))
        return PAMG_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAMG_ERR_NODEV;
    if (p->device < 0 || p->device >= ndev) return PAMG_ERR_NODEV;
    auto *h = new pamg_handle;
    h->p = *p;
    h->device = p->device;
    // PAMG_STREAM_CU_MASK=<n> | half (tests): the handle's stream runs on the first n CUs only (hipExtStreamCreateWithCUMask)
    // -- a persistent chain grid sized for every CU is then not co-resident (the chain's fail-safe path)
    const char *cm = getenv("PAMG_STREAM_CU_MASK");
    int ncu_mask = cm ? atoi(cm) : 0;
    if (cm && std::strcmp(cm, "half") == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, p->device) != hipSuccess) n = 0;
        ncu_mask = n / 2;
    }
    auto make_stream = [&](hipStream_t *st) -> bool {
        if (ncu_mask <= 0) return hipStreamCreateWithFlags(st, hipStreamNonBlocking) == hipSuccess;
        std::vector<uint32_t> mask((size_t)(ncu_mask + 31) / 32, 0u);
        for (int c = 0; c < ncu_mask; ++c) mask[c / 32] |= 1u << (c % 32);
        return hipExtStreamCreateWithCUMask(st, (uint32_t)mask.size(), mask.data()) == hipSuccess;
    };
    if (hipSetDevice(h->device) != hipSuccess || !make_stream(&h->stream) ||
        hipStreamCreateWithFlags(&h->stream_comm, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_packed, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_sent[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_sent[1], hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream_c, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fine, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_coarse, hipEventDisableTiming) != hipSuccess) {
        delete h;
        return PAMG_ERR_HIP;
    }
    *out = h;
    return PAMG_OK;
}

int pamg_upload_mesh(pamg_handle *h, int U, const double *X, const int *region, const int *neig, const int *fneig,
                     const int *dir) {
    if (!h || U < 1 || !X || !region || !neig || !fneig || !dir) return PAMG_ERR_ARG;
    CHK(settle(h));
    HIPCHK(h, hipSetDevice(h->device));
    if (h->agg) {
        (void)pamg_destroy(h->agg);
        h->agg = nullptr;
    }
    free_levels(h);
    h->U_global = U;
    h->owned.clear();
    if (!h->owner.empty() && (int)h->owner.size() != U) {
        h->err = "owner map size differs from the uploaded mesh";
        return PAMG_ERR_ARG;
    }
    if (!h->owner.empty()) {
        for (int g = 0; g < U; ++g) {
            if (h->owner[g] < 0 || h->owner[g] >= h->nranks) { h->err = "owner out of range"; return PAMG_ERR_ARG; }
            if (h->owner[g] == h->rank) h->owned.push_back(g);
        }
    } else {
        for (int g = 0; g < U; ++g) h->owned.push_back(g);
    }
    h->U = (int)h->owned.size();
    h->Xo.resize(6 * h->owned.size());
    for (size_t q = 0; q < h->owned.size(); ++q)
        for (int c = 0; c < 6; ++c) h->Xo[6 * q + c] = X[6 * (size_t)h->owned[q] + c];
    h->neig_local.clear();
    if (h->p.op == 1) {   // the local neighbours: the chain's workgroup lists
        std::vector<int> g2l(U, -1);
        for (size_t q = 0; q < h->owned.size(); ++q) g2l[h->owned[q]] = (int)q;
        h->neig_local.assign(3 * h->owned.size(), -1);
        for (size_t q = 0; q < h->owned.size(); ++q)
            for (int f = 0; f < 3; ++f) {
                const int n = neig[3 * (size_t)h->owned[q] + f];
                if (n >= 1 && n <= U) h->neig_local[3 * q + f] = g2l[n - 1];
            }
    }
    for (int g = 0; g < U; ++g)
        for (int f = 0; f < 3; ++f) {
            const int n = neig[3 * g + f];
            if (n < 0 || n > U || (n && (fneig[3 * g + f] < 1 || fneig[3 * g + f] > 3))) {
                h->err = "inconsistent neighbour table at un_ele " + std::to_string(g + 1);
                return PAMG_ERR_ARG;
            }
        }
    const int S = h->p.n_split, Lc = h->p.multi_levels, Ul = h->U;
    h->slots = (1 << S) * 3;
    CHK(dev_alloc(h, &h->tov, (size_t)h->slots * 3 * std::max(Ul, 1)));
    CHK(dev_alloc(h, &h->tovo, (size_t)h->slots * 3 * std::max(Ul, 1)));
    HIPCHK(h, hipMemsetAsync(h->tov, 0, (size_t)h->slots * 3 * std::max(Ul, 1) * sizeof(double), h->stream));
    HIPCHK(h, hipMemsetAsync(h->tovo, 0, (size_t)h->slots * 3 * std::max(Ul, 1) * sizeof(double), h->stream));
    // level-1 geometry for the source term
    {
        std::vector<double> geo((size_t)std::max(Ul, 1) * kGeoStride, 0.0);
        const double pw = (double)(1 << S);
        for (int q = 0; q < Ul; ++q) {
            const double *x = X + 6 * (size_t)h->owned[q];
            double *g = &geo[(size_t)q * kGeoStride];
            g[0] = x[4]; g[1] = x[5];
            g[2] = (x[0] - x[4]) / pw; g[3] = (x[1] - x[5]) / pw;
            g[4] = (x[2] - x[4]) / pw; g[5] = (x[3] - x[5]) / pw;
        }
        CHK(dev_upload(h, &h->geo1, geo));
    }
    std::vector<int> pos[kMaxLevels + 1];   // hierarchical storage order of every level (Level::pos)
    hier_positions(S, Lc, pos);
    for (int l = 1; l <= Lc; ++l) {
        std::vector<char> seen(pos[l].size(), 0);
        for (int v : pos[l])
            if (v < 0 || v >= (int)pos[l].size() || seen[v]++) { h->err = "storage order is not a permutation"; return PAMG_ERR_STATE; }
    }
    for (int l = 1; l <= Lc; ++l) {
        if (h->coarse_only && l < Lc) continue;   // a replica of the coarsest level (agg_create)
        Level &L = h->lv[l];
        L.pos = pos[l];
        L.isplit = S - l + 1;
        // the contracted arithmetic is for solvers 1 and 3; Richardson's residual keeps the
        // reference's order (as the oracle's get_residual)
        L.arith = h->p.solver == 2 ? 0 : h->p.arith;
        L.richardson = h->p.solver == 2;
        L.nsub = 1 << (2 * L.isplit);
        L.N = (int64_t)L.nsub * Ul;
        // (a gap between the planes, so that a sub-element's three are not a power-of-two distance apart, measured
        // within noise: profiles/r05_e_asm_layouts.txt)
        L.pitch = std::max<int64_t>(64, (L.N + 63) / 64 * 64);
        double *base = nullptr;
        // level 1: the source term s' (SRC); level 2: RHSN_alt for the concurrent fused cycle and the face cycle's
        // level-1 restrictor fold, levels 3 .. L: RHSN_alt for the face cycle's folds of the coarser levels
        const size_t planes = 21;
        CHK(dev_alloc(h, &base, planes * (size_t)L.pitch));
        HIPCHK(h, hipMemsetAsync(base, 0, planes * (size_t)L.pitch * sizeof(double), h->stream));
        L.T = base; L.TNN = base + 3 * L.pitch; L.RHS = base + 6 * L.pitch; L.RES = base + 9 * L.pitch;
        L.TOLD = base + 12 * L.pitch;
        L.RHSN = base + 15 * L.pitch;   // restriction of the zero residual: valid
        L.RHSN_alt = (l >= 2) ? base + 18 * L.pitch : nullptr;
        L.SRC = (l == 1) ? base + 18 * L.pitch : nullptr;
        std::vector<double> stc((size_t)std::max(Ul, 1) * kStcStride, 0.0);
        for (int q = 0; q < Ul; ++q) {
            level_stencil(X + 6 * (size_t)h->owned[q], L.isplit, h->p.k, h->p.dt, h->p.omega,
                          &stc[(size_t)q * kStcStride]);
            if (!mass_is_p1_midpoint(&stc[(size_t)q * kStcStride])) {
                h->err = "mass matrix of un_ele " + std::to_string(h->owned[q] + 1) + " is not c*[[2,1,1],[1,2,1],[1,1,2]]";
                return PAMG_ERR_STATE;
            }
        }
        CHK(dev_upload(h, &L.stc, stc));
        std::vector<int2> sub(L.nsub);
        for (int e = 1; e <= L.nsub; ++e) {
            int irow, ipos, o;
            get_str_info(L.isplit, e, &irow, &ipos, &o);
            sub[L.pos[e - 1]] = make_int2(irow, ipos);
        }
        CHK(dev_upload(h, &L.subinfo, sub));
        CHK(dev_upload(h, &L.d_pos, L.pos));
        if (l == 1) HIPCHK(h, launch_source(h->stream, L, h->geo1, h->p.k));   // s' of get_RHS, once
        CHK(build_halo(h, l, X, neig, fneig, dir));
        if (h->p.op == 1) {
            std::vector<int4> fnb;
            std::vector<double> fface;
            std::vector<int> fsx;
            CHK(build_face(h, l, X, neig, fneig, dir, fnb, fface, fsx));
            CHK(dev_upload(h, &L.fnb, fnb));
            CHK(dev_upload(h, &L.fface, fface));
            CHK(dev_upload(h, &L.fsx, fsx));
            // the up positions without halo words, the up ones with words, then the down ones (the
            // order inside a colour is free: a colour pass reads only the other colour)
            auto has_words = [&](int j) {
                if (j >= (int)L.halo.hsub.size()) return false;
                const int4 e = L.halo.hsub[j];
                return (e.x | e.y | e.z) != 0;
            };
            std::vector<int> cpos;
            L.nui = 0;
            for (int pass = 0; pass < 3; ++pass)
                for (int j = 0; j < L.nsub; ++j) {
                    const bool up = fnb[j].w != 0;
                    if (pass == 0 ? up && !has_words(j) : pass == 1 ? up && has_words(j) : !up) cpos.push_back(j);
                    if (pass == 0 && up && !has_words(j)) ++L.nui;
                }
            L.nup = 0;
            for (int j = 0; j < L.nsub; ++j) L.nup += fnb[j].w != 0;
            L.ndn = L.nsub - L.nup;
            L.words_up = true;
            for (int j = 0; j < L.nsub && j < (int)L.halo.hsub.size(); ++j) {
                const int4 e = L.halo.hsub[j];
                if ((e.x | e.y | e.z) && !fnb[j].w) L.words_up = false;
            }
            CHK(dev_upload(h, &L.cpos, cpos));
            std::vector<int4> cnb(cpos.size());
            for (size_t i = 0; i < cpos.size(); ++i) cnb[i] = fnb[cpos[i]];
            CHK(dev_upload(h, &L.cnb, cnb));
            // the two-sweep passes' gather table (k_face_pp, Level::gtab): for every halo slot of every local
            // un_ele, the neighbour's boundary sub-element e whose words fill it (hface: this un_ele's words
            // into the neighbour; the neighbour's record back: its words into this one, reversed or not) and,
            // for each face of e, where the value across it lives
            if (face_tile_shape(L)) {
                const int m = 1 << L.isplit, sl = h->slots, ns = L.nsub;
                std::vector<int4> gf((size_t)std::max(Ul, 1) * 3, make_int4(-1, 0, 0, 0));   // {v, fv, rev v->u, rev u->v}
                for (int q = 0; q < Ul; ++q)
                    for (int f = 1; f <= 3; ++f) {
                        const int4 r = L.halo.hface[3 * (size_t)q + f - 1];
                        const int mode = r.x & 3;
                        if (mode == 0) continue;
                        if (mode == 2) { gf[3 * (size_t)q + f - 1] = make_int4(-2, 0, 0, 0); continue; }
                        const int v = r.y / (3 * sl), fv = (r.y - v * 3 * sl) / sl + 1;
                        const int4 rv = L.halo.hface[3 * (size_t)v + fv - 1];
                        if ((rv.x & 3) != 1 || rv.y != q * 3 * sl + (f - 1) * sl) {
                            h->err = "face operator: asymmetric halo records between un_eles " + std::to_string(q) + " and " + std::to_string(v);
                            return PAMG_ERR_STATE;
                        }
                        gf[3 * (size_t)q + f - 1] = make_int4(v, fv, rv.x >> 2, r.x >> 2);
                    }
                std::vector<int> E(3 * (size_t)m, -1);   // boundary sub-element at position i of face f
                for (int j = 0; j < ns && j < (int)L.halo.hsub.size(); ++j) {
                    const int4 e = L.halo.hsub[j];
                    if (e.x) E[e.x - 1] = j;
                    if (e.y) E[m + e.y - 1] = j;
                    if (e.z) E[2 * m + e.z - 1] = j;
                }
                for (int v : E)
                    if (v < 0) { h->err = "face operator: a face position without its boundary sub-element"; return PAMG_ERR_STATE; }
                static const int fmface[3] = {1, 3, 2};   // un_ele face under sub-element face fi (pamg_face.hip cFMface)
                std::vector<int4> gt((size_t)std::max(Ul, 1) * 3 * m, make_int4(-1, 0, 0, 0));
                std::vector<int> gp(gt.size(), 0);
                for (int q = 0; q < Ul; ++q)
                    for (int f = 1; f <= 3; ++f) {
                        const int4 g = gf[3 * (size_t)q + f - 1];
                        for (int sp = 1; sp <= m; ++sp) {
                            int4 &o = gt[(3 * (size_t)q + f - 1) * m + sp - 1];
                            if (g.x < 0) { o = make_int4(g.x, 0, 0, 0); continue; }
                            const int e = E[(g.y - 1) * m + (g.z ? m - sp + 1 : sp) - 1];
                            const int4 nb = fnb[e];
                            const int nbf[3] = {nb.x, nb.y, nb.z};
                            int y[3];
                            for (int fi = 0; fi < 3; ++fi) {
                                if (nbf[fi] >= 0) { y[fi] = g.x * ns + nbf[fi]; continue; }
                                const int mf = fmface[fi], spp = -nbf[fi];
                                if (mf == g.y) {   // across to this un_ele: its own boundary sub-element
                                    y[fi] = -1 - E[(f - 1) * m + (g.w ? m - spp + 1 : spp) - 1];
                                    continue;
                                }
                                const int4 g2 = gf[3 * (size_t)g.x + mf - 1];   // a corner: the neighbour's other face
                                if (g2.x >= 0) y[fi] = g2.x * ns + E[(g2.y - 1) * m + (g2.z ? m - spp + 1 : spp) - 1];
                                else if (g2.x == -1)
                                    y[fi] = -(1 + ns + 3 * (L.halo.hface[3 * (size_t)g.x + mf - 1].z + spp - 1) + mf - 1);
                                else y[fi] = -1 - e;   // another rank: k_face_pp is single-domain (never read)
                            }
                            o = make_int4(g.x * ns + e, y[0], y[1], y[2]);
                            gp[(3 * (size_t)q + f - 1) * m + sp - 1] = (nb.x >= 0) | ((nb.y >= 0) << 1) | ((nb.z >= 0) << 2);
                        }
                    }
                CHK(dev_upload(h, &L.gtab, gt));
                CHK(dev_upload(h, &L.gpat, gp));
            }
        }
        HaloPlan &P = L.halo;
        CHK(dev_upload(h, &P.d_local, P.local));
        CHK(dev_upload(h, &P.d_bc, P.bc));
        CHK(dev_upload(h, &P.d_remote, P.remote));
        CHK(dev_upload(h, &P.d_recv_dst, P.recv_dst));
        CHK(dev_upload(h, &P.d_hface, P.hface));
        CHK(dev_upload(h, &P.d_hsub, P.hsub));
        {
            std::vector<int> bpos;
            for (int q = 0; q < (int)P.hsub.size(); ++q)
                if (P.hsub[q].x | P.hsub[q].y | P.hsub[q].z) bpos.push_back(q);
            P.nbpos = (int)bpos.size();
            if (bpos.empty()) bpos.push_back(0);
            CHK(dev_upload(h, &P.d_bpos, bpos));
        }
        CHK(dev_upload(h, &P.d_bcv, P.bcv));
        CHK(dev_upload(h, &P.d_surf, P.surf));
        CHK(dev_alloc(h, &P.d_told_halo, 3 * (size_t)P.n_told));
        CHK(refresh_told_halo(h, l));
        CHK(dev_alloc(h, &P.d_send, 6 * P.remote.size()));
        if (l == 1 && !P.remote.empty()) CHK(dev_alloc(h, &P.d_send_b, 6 * P.remote.size()));
        CHK(dev_alloc(h, &P.d_recv, 6 * P.recv_dst.size()));
    }
    // initial condition (:237-252): tnew = 0, region 4 => 1 on level 1
    if (!h->coarse_only) {
        Level &L1 = h->lv[1];
        bool any = false;
        for (int q = 0; q < Ul; ++q) any |= region[h->owned[q]] == 4;
        if (any) {
            std::vector<double> t(3 * (size_t)L1.pitch, 0.0);
            for (int q = 0; q < Ul; ++q)
                if (region[h->owned[q]] == 4)
                    for (int c = 0; c < 3; ++c)
                        for (int e = 0; e < L1.nsub; ++e) t[c * L1.pitch + (size_t)q * L1.nsub + e] = 1.0;
            // behind the memset of the level's planes on the same stream
            HIPCHK(h, hipMemcpyAsync(L1.T, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        HIPCHK(h, launch_copy(h->stream, L1.T, L1.TNN, 3 * L1.pitch));
        h->tnn_level = 1;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->mesh_ready = true;
    return agg_create(h, U, X, region, neig, fneig, dir);
}

int pamg_owned_count(pamg_handle *h) { return h ? h->U : PAMG_ERR_ARG; }

int pamg_nsub(pamg_handle *h, int level) {
    if (!h) return PAMG_ERR_ARG;
    CHK(check_level(h, level));
    return h->lv[level].nsub;
}

int pamg_tnn_level(pamg_handle *h) { return h ? h->tnn_level : PAMG_ERR_ARG; }

int pamg_set_state(pamg_handle *h, int level, int what, const double *host) {
    if (!h || !host) return PAMG_ERR_ARG;
    CHK(settle(h));
    if (what == PAMG_TNEW_NONLIN) { CHK(check_level(h, level)); h->tnn_level = level; }
    CHK(check_level(h, level));
    Level &L = h->lv[level];
    // the source is read-only, and so is the error: only pamg_get_error writes it
    double *dst = what == PAMG_SOURCE || what == PAMG_ERROR ? nullptr : field_ptr(h, level, what);
    if (!dst) return PAMG_ERR_ARG;
    CHK(ensure_scratch(h, 3 * (size_t)L.N * sizeof(double)));
    HIPCHK(h, hipMemcpyAsync(h->scratch, host, 3 * (size_t)L.N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_to_soa(h->stream, L, h->scratch, dst));
    if (what == PAMG_TOLD) CHK(refresh_told_halo(h, level));
    if (what == PAMG_RESIDUAL) h->rhsn_valid = false;
    CHK(sync_stream(h, h->stream));
    return PAMG_OK;
}

int pamg_get_state(pamg_handle *h, int level, int what, double *host) {
    if (!h || !host) return PAMG_ERR_ARG;
    CHK(settle(h));
    if (what == PAMG_TNEW_NONLIN) level = h->tnn_level;
    CHK(check_level(h, level));
    Level &L = h->lv[level];
    if (what == PAMG_ERROR && level == 1) CHK(error_setup(h));
    double *src = field_ptr(h, level, what);
    if (!src) return PAMG_ERR_ARG;
    CHK(ensure_scratch(h, 3 * (size_t)L.N * sizeof(double)));
    HIPCHK(h, launch_to_aos(h->stream, L, src, h->scratch));
    HIPCHK(h, hipMemcpyAsync(host, h->scratch, 3 * (size_t)L.N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CHK(sync_stream(h, h->stream));
    return PAMG_OK;
}

int pamg_get_overlap(pamg_handle *h, double *tov, double *tovo) {
    if (!h || !h->mesh_ready) return PAMG_ERR_STATE;
    CHK(settle(h));
    const size_t n = (size_t)h->slots * 3 * h->U * sizeof(double);
    if (tov) HIPCHK(h, hipMemcpyAsync(tov, h->tov, n, hipMemcpyDeviceToHost, h->stream));
    if (tovo) HIPCHK(h, hipMemcpyAsync(tovo, h->tovo, n, hipMemcpyDeviceToHost, h->stream));
    CHK(sync_stream(h, h->stream));
    return PAMG_OK;
}

int pamg_begin_timestep(pamg_handle *h) {
    if (!h) return PAMG_ERR_ARG;
    CHK(settle(h));
    return begin_timestep(h, false);
}

int pamg_copy_to_nonlin(pamg_handle *h, int level) {
    if (!h) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, level));
    Level &L = h->lv[level];
    HIPCHK(h, launch_copy(h->stream, L.T, L.TNN, 3 * L.pitch));
    h->tnn_level = level;
    return PAMG_OK;
}

int pamg_smoother(pamg_handle *h, int level, int n_calls) {
    if (!h || n_calls < 0) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, level));
    if (h->tnn_level != level) {
        h->err = "smoother: tnew_nonlin holds another level (call pamg_copy_to_nonlin first)";
        return PAMG_ERR_STATE;
    }
    CHK(smooth(h, level, false, h->p.n_smooth * n_calls));
    return h->p.op == 1 ? face_chain_check(h) : PAMG_OK;
}

int pamg_sweep(pamg_handle *h, int level, int n_sweeps) {
    if (!h || n_sweeps < 0) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, level));
    if (h->tnn_level != level) {
        h->err = "sweep: tnew_nonlin holds another level (call pamg_copy_to_nonlin first)";
        return PAMG_ERR_STATE;
    }
    CHK(smooth(h, level, false, n_sweeps));
    return h->p.op == 1 ? face_chain_check(h) : PAMG_OK;
}

int pamg_restrictor(pamg_handle *h, int level) {
    if (!h) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, level));
    return restrict_(h, level);
}

int pamg_get_residual(pamg_handle *h, int level) {
    if (!h) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, level));
    return residual(h, level);
}

int pamg_prolongator(pamg_handle *h, int level) {
    if (!h) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, level));
    return prolong(h, level, false);
}

int pamg_vcycle(pamg_handle *h, int n) {
    if (!h || n < 0) return PAMG_ERR_ARG;
    CHK(vcycle(h, n, false));
    return comm_error(h);
}

int pamg_field_norm(pamg_handle *h, int level, int what, int kind, double *value) {
    if (!h || !value) return PAMG_ERR_ARG;
    if (!field_kind_ok(kind)) { h->err = "norm: unknown kind"; return PAMG_ERR_ARG; }
    CHK(settle(h));
    if (what == PAMG_TNEW_NONLIN) level = h->tnn_level;   // as pamg_get_state
    CHK(check_level(h, level));
    CHK(norm_level_ok(h, level));
    if (what == PAMG_ERROR && level == 1) CHK(error_setup(h));
    const double *src = field_ptr(h, level, what);
    if (!src) { h->err = "norm: no such field on this level"; return PAMG_ERR_ARG; }
    NormRec r;
    CHK(norm_reduce(h, level, src, kFormField, norm_mode(kind), &r));
    *value = norm_value(r, kind);
    return PAMG_OK;
}

// `call get_error` (:303, body :531-540): tracer(1)%error := |tnew - analytical| on level 1; nothing else is written
int pamg_get_error(pamg_handle *h) {
    if (!h) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, 1));
    CHK(error_setup(h));
    Level &L = h->lv[1];
    if (L.N == 0) return PAMG_OK;   // a rank that owns nothing
    Span sp(h, PAMG_K_NORM, 48.0 * (double)L.N);
    HIPCHK(h, launch_error(h->stream, L, h->geo1, L.ERR));
    return PAMG_OK;
}

int pamg_error_norm(pamg_handle *h, int kind, double *value) {
    if (!h || !value) return PAMG_ERR_ARG;
    if (!field_kind_ok(kind)) { h->err = "norm: unknown kind"; return PAMG_ERR_ARG; }
    CHK(settle(h));
    CHK(check_level(h, 1));
    NormRec r;
    CHK(norm_reduce(h, 1, nullptr, kFormError, norm_mode(kind), &r));
    *value = norm_value(r, kind);
    return PAMG_OK;
}

int pamg_get_convergence(pamg_handle *h, int level, double *convergence) {
    if (!h || !convergence) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, level));
    CHK(norm_level_ok(h, level));
    CHK(residual(h, level));   // `call get_residual(ilevel)` (:877)
    NormRec r;
    CHK(norm_reduce(h, level, h->lv[level].RES, kFormField, 0, &r));
    *convergence = norm_value(r, PAMG_NORM_REF);
    return PAMG_OK;
}

int pamg_residual_norm(pamg_handle *h, int level, int kind, double *value) {
    if (!h || !value) return PAMG_ERR_ARG;
    if (!norm_kind_ok(kind)) { h->err = "norm: unknown kind"; return PAMG_ERR_ARG; }
    CHK(residual_norm_ok(h));
    CHK(settle(h));
    CHK(check_level(h, level));
    CHK(norm_level_ok(h, level));
    return residual_norm(h, level, kind, value);
}

int pamg_solve(pamg_handle *h, int kind, double tol, int max_cycles, int check_every, int *cycles, double *value,
               int *status, double *history, int history_len, int *n_history) {
    if (!h) return PAMG_ERR_ARG;
    if (!norm_kind_ok(kind)) { h->err = "solve: unknown kind"; return PAMG_ERR_ARG; }
    if (max_cycles < 0 || check_every < 1 || history_len < 0 || (history_len > 0 && !history)) {
        h->err = "solve: max_cycles >= 0, check_every >= 1 and a history array of history_len entries are required";
        return PAMG_ERR_ARG;
    }
    CHK(residual_norm_ok(h));
    CHK(check_level(h, 1));
    int done = 0, checks = 0, st = PAMG_SOLVE_MAXCYCLES;
    double v = std::nan("");
    while (done < max_cycles) {
        const int n = std::min(check_every, max_cycles - done);
        CHK(vcycle(h, n, false));   // pamg_vcycle(n)
        CHK(comm_error(h));
        done += n;
        CHK(settle(h));
        CHK(residual_norm(h, 1, kind, &v));
        if (checks < history_len) history[checks] = v;
        ++checks;
        if (!std::isfinite(v)) { st = PAMG_SOLVE_NONFINITE; break; }
        if (v <= tol) { st = PAMG_SOLVE_CONVERGED; break; }
    }
    if (cycles) *cycles = done;
    if (value) *value = v;
    if (status) *status = st;
    if (n_history) *n_history = checks;
    return PAMG_OK;
}

int pamg_direct_solve(pamg_handle *h, int level) {
    if (!h) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, level));
    return direct_solve(h, level);
}

int pamg_block_inverse(pamg_handle *h, int n, long nb, const double *A, double *inv, int *errorflag) {
    if (!h || n < 1 || n > 8 || nb < 0 || (nb > 0 && (!A || !inv || !errorflag))) return PAMG_ERR_ARG;
    if (nb == 0) return PAMG_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t nd = (size_t)n * n * (size_t)nb;
    double *dA = nullptr, *dI = nullptr;
    int *dE = nullptr;
    int rc = PAMG_OK;
    if (hipMalloc((void **)&dA, nd * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&dI, nd * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&dE, (size_t)nb * sizeof(int)) != hipSuccess ||
        hipMemcpyAsync(dA, A, nd * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        launch_block_inverse(h->stream, n, nb, dA, dI, dE) != hipSuccess ||
        hipMemcpyAsync(inv, dI, nd * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(errorflag, dE, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
        h->err = "pamg_block_inverse: HIP error";
        rc = PAMG_ERR_HIP;
    }
    (void)hipFree(dA);
    (void)hipFree(dI);
    (void)hipFree(dE);
    return rc;
}

int pamg_run(pamg_handle *h, int ntime, int n_multigrid) {
    if (!h || ntime < 0 || n_multigrid < 0) return PAMG_ERR_ARG;
    CHK(settle(h));
    {
        // the resident schedule runs the whole loop as one launch: a step touches only its own
        // tiles (told := tnew, the RHS from it and s', n_multigrid cycles), so every tile goes
        // through all ntime steps on-chip and only the run's final state is stored
        const int L = h->p.multi_levels;
        if (ntime >= 2 && n_multigrid >= 1 && h->p.cycle == 0 && h->p.fused == 3 && h->p.coarse_solver == 0 &&
            h->p.op == 0 && h->p.halo_exchange == 0 && !h->coarse_ahead && call_schedule(h) == 3 && fused_ok(h) &&
            vcycle_resident_run_supported(h->p.n_split, L) && vcycle_rhsf_supported(h->p.n_split) &&
            !PAMG_RHS_TOLD_HALO) {
            int rc = begin_timestep(h, true, true, true);
            if (rc == PAMG_OK) rc = vcycle_fused(h, n_multigrid, false, ntime);
            if (rc != PAMG_OK) {
                h->coarse_ahead = false;
                h->rhs_pending = false;
                return rc;
            }
            return comm_error(h);
        }
    }
    for (int t = 0; t < ntime; ++t) {
        const int L = h->p.multi_levels;
        const bool fused_next = n_multigrid > 0 && fused_ok(h);
        // told := tnew and the RHS inside the step's first level-1 launch when that launch is a
        // pipelined one on the one-stream schedule
        // (the resident schedule starts the step in its one launch, for any n_multigrid)
        const int cs = call_schedule(h);
        const bool defer_rhs = fused_next && h->p.fused == 3 && L > 1 && h->p.halo_exchange == 0 &&
                               vcycle_rhsf_supported(h->p.n_split) &&
                               (cs == 3 ? vcycle_resident_supported(h->p.n_split, L)
                                        : cs == 1 && (n_multigrid > 1 || t + 1 < ntime)) &&
                               !PAMG_RHS_TOLD_HALO;
        int rc = begin_timestep(h, n_multigrid > 0 && h->p.cycle == 0, fused_next, defer_rhs);
        if (rc == PAMG_OK) rc = vcycle(h, n_multigrid, t + 1 < ntime);   // a step's leftovers die in the next one
        if (rc != PAMG_OK) {
            h->coarse_ahead = false;
            h->rhs_pending = false;
            return rc;
        }
    }
    return comm_error(h);
}

int pamg_synchronize(pamg_handle *h) {
    if (!h) return PAMG_ERR_ARG;
    CHK(sync_stream(h, h->stream));
    if (h->sent_pending[0] || h->sent_pending[1]) CHK(sync_stream(h, h->stream_comm));
    return PAMG_OK;
}

int pamg_timing_enable(pamg_handle *h, unsigned mask) {
    if (!h) return PAMG_ERR_ARG;
    h->timing.mask = mask;
    return PAMG_OK;
}

int pamg_early_exchange_times(pamg_handle *h, double t[3]) {
    if (!h || !t) return PAMG_ERR_ARG;
    if (!h->xe_ev_valid) return PAMG_ERR_STATE;
    CHK(sync_stream(h, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream_comm));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, h->xe_ev[0], h->xe_ev[k + 1]));
        t[k] = 1e3 * (double)ms;
    }
    return PAMG_OK;
}

int pamg_timing_reset(pamg_handle *h) {
    if (!h) return PAMG_ERR_ARG;
    h->xe_ev_valid = false;
    CHK(drain_timing(h));
    for (int k = 0; k < PAMG_K_COUNT; ++k) {
        h->timing.ms[k] = 0; h->timing.count[k] = 0; h->timing.bytes[k] = 0; h->timing.seq[k] = 0;
    }
    return PAMG_OK;
}

int pamg_vcycle_flops(pamg_handle *h, double *flops_per_cycle) {
    if (!h || !flops_per_cycle) return PAMG_ERR_ARG;
    if (!h->mesh_ready) return PAMG_ERR_STATE;
    *flops_per_cycle = vcycle_flops(h);
    return PAMG_OK;
}

int pamg_set_call_schedule(pamg_handle *h, int schedule) {
    if (!h || schedule < 0 || schedule > 3) return PAMG_ERR_ARG;
    h->call_schedule = schedule;
    return PAMG_OK;
}

int pamg_timing_stride(pamg_handle *h, int every) {
    if (!h || every < 1) return PAMG_ERR_ARG;
    h->timing.stride = every;
    return PAMG_OK;
}

int pamg_timing_read(pamg_handle *h, int kid, double *ms_total, long *launches, double *bytes_total) {
    if (!h || kid < 0 || kid >= PAMG_K_COUNT) return PAMG_ERR_ARG;
    CHK(drain_timing(h));
    if (ms_total) *ms_total = h->timing.ms[kid];
    if (launches) *launches = h->timing.count[kid];
    if (bytes_total) *bytes_total = h->timing.bytes[kid];
    return PAMG_OK;
}

int pamg_timing_issued(pamg_handle *h, int kid, long *issued) {
    if (!h || !issued || kid < 0 || kid >= PAMG_K_COUNT) return PAMG_ERR_ARG;
    *issued = h->timing.seq[kid];
    return PAMG_OK;
}

int pamg_sweep_bench(pamg_handle *h, int sweeps, int assembled, double *ms_avg, double *bytes_per_launch) {
    if (!h || sweeps < 1) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, 1));
    Level &L = h->lv[1];
    const double rdt = 1 / h->p.dt;
    CHK(ensure_scratch(h, 3 * (size_t)L.pitch * sizeof(double)));
    if (assembled && !L.blocks) {
        CHK(dev_alloc(h, &L.blocks, asm_blocks_doubles(L)));
        HIPCHK(h, launch_build_blocks(h->stream, L, rdt));
    }
    const double bytes = assembled ? 168.0 * (double)L.N : 72.0 * (double)L.N + 168.0 * h->U;
    const unsigned saved = h->timing.mask;
    CHK(drain_timing(h));
    const double ms0 = h->timing.ms[PAMG_K_SWEEP_BENCH];
    const long n0 = h->timing.count[PAMG_K_SWEEP_BENCH];
    h->timing.mask |= 1u << PAMG_K_SWEEP_BENCH;
    for (int s = 0; s < sweeps; ++s) {
        Span sp(h, PAMG_K_SWEEP_BENCH, bytes);
        if (assembled) HIPCHK(h, launch_sweep_assembled(h->stream, L, h->scratch, rdt));
        else HIPCHK(h, launch_sweep_stencil(h->stream, L, h->scratch, rdt));
    }
    h->timing.mask = saved;
    CHK(drain_timing(h));
    const long n = h->timing.count[PAMG_K_SWEEP_BENCH] - n0;
    if (ms_avg) *ms_avg = (h->timing.ms[PAMG_K_SWEEP_BENCH] - ms0) / std::max(1L, n);
    if (bytes_per_launch) *bytes_per_launch = bytes;
    return PAMG_OK;
}

int pamg_sweep_bench_output(pamg_handle *h, int assembled, double *host) {
    if (!h || !host) return PAMG_ERR_ARG;
    CHK(settle(h));
    CHK(check_level(h, 1));
    Level &L = h->lv[1];
    const double rdt = 1 / h->p.dt;
    // the sweep's output planes, then its (3, nsub, U) image
    CHK(ensure_scratch(h, 6 * (size_t)L.pitch * sizeof(double)));
    if (assembled && !L.blocks) {
        CHK(dev_alloc(h, &L.blocks, asm_blocks_doubles(L)));
        HIPCHK(h, launch_build_blocks(h->stream, L, rdt));
    }
    if (assembled) HIPCHK(h, launch_sweep_assembled(h->stream, L, h->scratch, rdt));
    else HIPCHK(h, launch_sweep_stencil(h->stream, L, h->scratch, rdt));
    double *img = h->scratch + 3 * L.pitch;
    HIPCHK(h, launch_to_aos(h->stream, L, h->scratch, img));
    HIPCHK(h, hipMemcpyAsync(host, img, 3 * (size_t)L.N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CHK(sync_stream(h, h->stream));
    return PAMG_OK;
}

int pamg_last_error(pamg_handle *h, char *buf, int len) {
    if (!h || !buf || len <= 0) return PAMG_ERR_ARG;
    std::strncpy(buf, h->err.c_str(), (size_t)len - 1);
    buf[len - 1] = 0;
    return PAMG_OK;
}

int pamg_destroy(pamg_handle *h) {
    if (!h) return PAMG_OK;
    (void)hipSetDevice(h->device);
    (void)face_gates_drain(h);
    if (h->agg) {
        (void)pamg_destroy(h->agg);
        h->agg = nullptr;
    }
    (void)hipStreamSynchronize(h->stream);
    if (h->stream_fb) (void)hipStreamSynchronize(h->stream_fb);
    (void)hipStreamSynchronize(h->stream_comm);
    if (h->stream_c) (void)hipStreamSynchronize(h->stream_c);
    free_levels(h);
    dev_free(h->scratch);
    dev_free(h->chain_tmo);
    if (h->gate) (void)hipFree(h->gate);
    if (h->gate_stat) (void)hipHostFree(h->gate_stat);
    if (h->norm_host) (void)hipHostFree(h->norm_host);
    if (h->stream_fb) (void)hipStreamDestroy(h->stream_fb);
    dev_free(h->xc_done);
    dev_free(h->xe_done);
    for (auto e : h->xe_ev)
        if (e) (void)hipEventDestroy(e);
    if (h->xc_sig) (void)hipFree(h->xc_sig);
    for (auto e : h->timing.pool) (void)hipEventDestroy(e);
    for (auto &r : h->timing.pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    if (h->borrowed_stream) {   // a coarsest-level replica: the streams are its parent's
        delete h;
        return PAMG_OK;
    }
    if (h->comm) {
        if (h->comm->nccl) nccl_release(h->comm->nccl);
        if (h->comm->ev_ready) (void)hipEventDestroy(h->comm->ev_ready);
        if (h->comm->ev_done) (void)hipEventDestroy(h->comm->ev_done);
        if (LocalGroup *G = h->comm->local) {
            bool last;
            {
                std::lock_guard<std::mutex> lk(G->mu);
                last = --G->refs == 0;
            }
            if (last) delete G;
        }
        delete h->comm;
    }
    (void)hipStreamSynchronize(h->stream_comm);
    if (h->stream_c) (void)hipStreamSynchronize(h->stream_c);
    for (hipEvent_t e : {h->ev_packed, h->ev_sent[0], h->ev_sent[1], h->ev_fine, h->ev_coarse})
        if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(h->stream_comm);
    if (h->stream_c) (void)hipStreamDestroy(h->stream_c);
    if (!h->borrowed_stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return PAMG_OK;
}

}  // extern "C"
