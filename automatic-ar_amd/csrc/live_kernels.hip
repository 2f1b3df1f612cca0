// Live tracker: frames arrive one per push; the last lag + 1 of them (the window) are refined together, the frame that
// left the window last (the anchor) is held fixed,
//
//   E = sum_{f in window} E_f(z_f) + sum_{f, f+1 in window} e_f^T L_f e_f + [anchor] e_a^T L_a e_a,   e_a = e(z_anchor, z_first)
//
// with E_f track()'s frame error (track_eval.hpp) and e_f, L_f the smoothed tracker's between factor (pair_terms.hpp).  smooth = 0 drops every
// prior: the window is one frame and the loop is k_track's.
//
// k_live_push runs the WHOLE LM of one push in ONE workgroup of four wavefronts; the phases are separated by workgroup barriers and hand
// over through LDS:
//   assembly   wavefront w takes the window frames w, w + 4, ...: V_f, g_f, E_f by track_eval, then the between factors of the pair that
//              ends at the frame (its J_b half; for the first frame that is the anchor pair) and of the pair that starts there (its J_a half
//              and the off-diagonal block) -> H_ff, H_{f,f+1}, b_f, the costs
//   solve      wavefront 0, every lane the same registers: (H + mu I) delta = b by sequential block elimination, pivots inverted by
//              spd6_inverse; a non-positive pivot sets the flag
//   trial      the costs at z + delta, |delta_f|^2 and delta_f . b_f per frame
//   decide     every thread adds the per-frame values in window order and takes the same accept / mu / exit decision
// No atomics; every sum has one owner and a fixed order, so two trackers fed the same pushes give the same bits.
// k_live_push<true> adds the marginal prior in the anchor pair's place and, behind the LM, a tail: one fresh assembly at the
// final point, then on wavefront 0 the elimination at mu = 0, the marginal of the frame that leaves and the covariance blocks.
#include "geom.hpp"
#include "kernels.h"
#include "pair_terms.hpp"
#include "track_eval.hpp"

namespace aar {

namespace {

struct LiveShared {
    double D[LIVE_MAX_W][36], O[LIVE_MAX_W][36], inv[LIVE_MAX_W][36];   // H_ff, H_{f,f+1}, the inverted pivots of the last solve
    double b[LIVE_MAX_W][6], c[LIVE_MAX_W][6], dl[LIVE_MAX_W][6];       // b_f, the eliminated right-hand side, the step
    double z[LIVE_MAX_W][6], zt[LIVE_MAX_W][6];                         // the current point and the trial point
    double Ef[2][LIVE_MAX_W], Pe[2][LIVE_MAX_W];                        // costs of the two points; Pe[.][i]: the pair that ends at frame i
    double lin[LIVE_MAX_W][2];                                          // |delta_f|^2, delta_f . b_f
    double za[6];                                                       // the anchor
    int flag;                                                           // a non-positive pivot in the last solve
};

// a bank member's workgroup also keeps, by window position, what a single tracker has in its kernel arguments
struct LiveBankShared : LiveShared {
    int cnt[LIVE_MAX_W];                // LiveArgs::cnt, read from the window's slot headers
    double lam[LIVE_MAX_W][2];          // LiveArgs::lam, from the shared argument block
};

// the constant-velocity instance keeps, by window position, the expected motion (rvec, t) of the pair that ENDS at the
// frame (position 0: the anchor pair's): the caller copies them from the kernel arguments before the first barrier
struct LiveMotionShared : LiveShared {
    double rel[LIVE_MAX_W][6];
};
// ... and the same behind a bank member's cnt and lam (the gated single tracker refines as the one member of a bank)
struct LiveBankMotionShared : LiveBankShared {
    double rel[LIVE_MAX_W][6];
};

// what the tail instance adds
struct LiveTail {
    double Lm[36], m[6];                // the marginal prior on the first window frame
    double B[36], cB[6];                // the J_b half of pair (0, 1) alone: J_b^T L_1 J_b, -J_b^T L_1 e_0
    double S[LIVE_MAX_W][36];           // the diagonal blocks of H^-1
};

__device__ __forceinline__ const char *live_slot(const LiveArgs &a, int i) {
    int s = a.first_slot + i;
    if (s >= a.slots) s -= a.slots;
    return a.ring + (size_t)s * a.slot_bytes;
}

// a value every lane holds alike, into scalar registers
__device__ __forceinline__ unsigned long long uni64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
template <typename T>
__device__ __forceinline__ T *uni_ptr(T *p) { return reinterpret_cast<T *>(uni64(reinterpret_cast<unsigned long long>(p))); }
__device__ __forceinline__ double uni_f64(double v) { return __longlong_as_double((long long)uni64((unsigned long long)__double_as_longlong(v))); }

// the window's detection counts and pair weights: a single tracker has them in its kernel arguments; a bank member (BANK) in LDS, where its
// kernel put them (s is then a LiveBankShared) -- a member's LiveArgs is built in registers, which cannot be indexed by window position
template <bool BANK>
__device__ __forceinline__ int live_cnt(const LiveArgs &a, const LiveShared &s, int i) {
    if constexpr (BANK) return __builtin_amdgcn_readfirstlane(static_cast<const LiveBankShared &>(s).cnt[i]);
    else return a.cnt[i];
}
template <bool BANK>
__device__ __forceinline__ double live_lam(const LiveArgs &a, const LiveShared &s, int i, int k) {
    if constexpr (BANK) return static_cast<const LiveBankShared &>(s).lam[i][k];
    else return a.lam[i][k];
}

// the expected motion of the pair that ends at window frame i: none (the random walk) unless MOTION (s is then a LiveMotionShared)
template <bool BANK, bool MOTION>
__device__ __forceinline__ const double *live_rel(const LiveShared &s, int i) {
    if constexpr (MOTION && BANK) return static_cast<const LiveBankMotionShared &>(s).rel[i];
    else if constexpr (MOTION) return static_cast<const LiveMotionShared &>(s).rel[i];
    else return nullptr;
}

// WITH_J: H, b and the costs at s.z; else the costs at s.z + s.dl (-> s.zt) with the linear model's sums
template <bool WITH_J, bool BANK, bool MOTION>
__device__ __forceinline__ void live_eval(const LiveArgs &a, const TrackArgs &ta, LiveShared &s, int wv, int lane) {
    const int W = a.W, out = WITH_J ? 0 : 1;
    for (int i = wv; i < W; i += 4) {
        double zc[6], rowc[ENT_STRIDE];
        ld6(s.z[i], zc);
        if (!WITH_J) {
            double d[6];
            ld6(s.dl[i], d);
            double d2 = 0.0, dg = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                zc[k] += d[k];
                d2 += d[k] * d[k];
                dg += d[k] * s.b[i][k];
            }
            if (lane < 6) s.zt[i][lane] = s.z[i][lane] + s.dl[i][lane];
            if (lane == 0) { s.lin[i][0] = d2; s.lin[i][1] = dg; }
        }
        make_ent_row(zc, rowc);
        double V[21], g[6];
        const char *rec = live_slot(a, i) + LIVE_HDR_BYTES;
        const double Ef = track_eval_range<WITH_J, LIVE_REC_BYTES, LIVE_REC_BYTES>(ta, rec, rec + sizeof(ObsIdx), 0, live_cnt<BANK>(a, s, i), zc, lane, V, g);
        double D[6][6], b[6];
        if (WITH_J) {
#pragma unroll
            for (int k = 0; k < 6; k++) {
                b[k] = g[k];   // track_eval's g is already -J^T r_w
#pragma unroll
                for (int j = 0; j < 6; j++) D[k][j] = V[sym6(k, j)];
            }
        }
        // the pair that ends here: this frame is its b side; for the first window frame the a side is the anchor, a constant
        double Pe = 0.0;
        if (a.smooth && (i > 0 || a.anchor_pair)) {
            double zp[6], rowp[ENT_STRIDE];
            if (i > 0) {
                ld6(s.z[i - 1], zp);
                if (!WITH_J) {
#pragma unroll
                    for (int k = 0; k < 6; k++) zp[k] += s.dl[i - 1][k];
                }
            } else {
                ld6(s.za, zp);
            }
            make_ent_row(zp, rowp);
            double phi[3], et[3], Ma[9], Mb[9];
            pair_terms<WITH_J>(rowp, rowc, live_rel<BANK, MOTION>(s, i), phi, et, Ma, Mb);
            const double lr = live_lam<BANK>(a, s, i, 0), lt = live_lam<BANK>(a, s, i, 1);
            Pe = lr * (phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]) + lt * (et[0] * et[0] + et[1] * et[1] + et[2] * et[2]);
            if (WITH_J) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
#pragma unroll
                    for (int j = 0; j < 3; j++) D[k][j] += lr * (Mb[k] * Mb[j] + Mb[3 + k] * Mb[3 + j] + Mb[6 + k] * Mb[6 + j]);
                    D[3 + k][3 + k] += lt;
                    b[k] -= lr * (Mb[k] * phi[0] + Mb[3 + k] * phi[1] + Mb[6 + k] * phi[2]);
                    b[3 + k] -= lt * et[k];
                }
            }
        }
        // the pair that starts here: its a side and the off-diagonal block
        if (WITH_J && a.smooth && i + 1 < W) {
            double zn[6], rown[ENT_STRIDE];
            ld6(s.z[i + 1], zn);
            make_ent_row(zn, rown);
            double phi[3], et[3], Ma[9], Mb[9];
            pair_terms<true>(rowc, rown, live_rel<BANK, MOTION>(s, i + 1), phi, et, Ma, Mb);
            const double lr = live_lam<BANK>(a, s, i + 1, 0), lt = live_lam<BANK>(a, s, i + 1, 1);
            double O[36];
#pragma unroll
            for (int k = 0; k < 36; k++) O[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    D[k][j] += lr * (Ma[k] * Ma[j] + Ma[3 + k] * Ma[3 + j] + Ma[6 + k] * Ma[6 + j]);
                    O[6 * k + j] = lr * (Ma[k] * Mb[j] + Ma[3 + k] * Mb[3 + j] + Ma[6 + k] * Mb[6 + j]);
                }
                D[3 + k][3 + k] += lt;
                O[6 * (3 + k) + 3 + k] = -lt;
                b[k] -= lr * (Ma[k] * phi[0] + Ma[3 + k] * phi[1] + Ma[6 + k] * phi[2]);
                b[3 + k] += lt * et[k];
            }
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 36; k++) s.O[i][k] = O[k];
            }
        }
        if (lane == 0) {
            s.Ef[out][i] = Ef;
            s.Pe[out][i] = Pe;
            if (WITH_J) {
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    s.b[i][k] = b[k];
#pragma unroll
                    for (int j = 0; j < 6; j++) s.D[i][6 * k + j] = D[k][j];
                }
            }
        }
    }
}

// The marginal prior (z_0 - m)^T Lm (z_0 - m) on the first window frame, added by the wavefront that has just assembled that frame (wavefront 0,
// behind its live_eval: lane 0 wrote the entries it now reads).  Its Jacobian is the identity: D_0 += Lm, b_0 -= Lm (z_0 - m), Pe[0] = E_m.
template <bool WITH_J>
__device__ __forceinline__ void live_prior(LiveShared &s, const LiveTail &tl, int lane) {
    double e[6], Le[6], Pm = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) e[k] = (WITH_J ? s.z[0][k] : s.z[0][k] + s.dl[0][k]) - tl.m[k];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 6; j++) t = fma(tl.Lm[6 * k + j], e[j], t);
        Le[k] = t;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) Pm = fma(e[k], Le[k], Pm);
    if (lane == 0) {
        s.Pe[WITH_J ? 0 : 1][0] = Pm;   // (no anchor pair in this mode: the entry held 0)
        if (WITH_J) {
#pragma unroll
            for (int k = 0; k < 6; k++) s.b[0][k] -= Le[k];
#pragma unroll
            for (int k = 0; k < 36; k++) s.D[0][k] += tl.Lm[k];
        }
    }
}

// (H + mu I) delta = b, block tridiagonal, by one wavefront whose lanes all carry the same values (every lane writes what it later reads):
//   P_0 = D_0 + mu I,  T_f = O_{f-1}^T P_{f-1}^-1,  P_f = D_f + mu I - T_f O_{f-1},  c_f = b_f - T_f c_{f-1};  x_f = P_f^-1 (c_f - O_f x_{f+1})
__device__ __forceinline__ void live_solve(LiveShared &s, int W, double mu) {
    bool ok = true;
    double inv[36], c[6];
    for (int f = 0; f < W; f++) {
        double P[6][6], cn[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            cn[i] = s.b[f][i];
#pragma unroll
            for (int k = 0; k < 6; k++) P[i][k] = s.D[f][6 * i + k] + (i == k ? mu : 0.0);
        }
        if (f > 0) {
            double O[36], T[36];
#pragma unroll
            for (int i = 0; i < 36; i++) O[i] = s.O[f - 1][i];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    double t = 0.0;
#pragma unroll
                    for (int p = 0; p < 6; p++) t = fma(O[6 * p + i], inv[6 * p + k], t);
                    T[6 * i + k] = t;
                }
#pragma unroll
            for (int i = 0; i < 6; i++) {
#pragma unroll
                for (int k = 0; k <= i; k++) {
                    double t = 0.0;
#pragma unroll
                    for (int p = 0; p < 6; p++) t = fma(T[6 * i + p], O[6 * p + k], t);
                    P[i][k] -= t;
                    if (k != i) P[k][i] = P[i][k];
                }
                double t = 0.0;
#pragma unroll
                for (int p = 0; p < 6; p++) t = fma(T[6 * i + p], c[p], t);
                cn[i] -= t;
            }
        }
        ok = spd6_inverse(P, inv) && ok;
#pragma unroll
        for (int i = 0; i < 6; i++) c[i] = cn[i];
#pragma unroll
        for (int i = 0; i < 36; i++) s.inv[f][i] = inv[i];
#pragma unroll
        for (int i = 0; i < 6; i++) s.c[f][i] = c[i];
    }
    double x[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 6; j++) t += inv[6 * i + j] * c[j];
        x[i] = t;
        s.dl[W - 1][i] = t;
    }
    for (int f = W - 2; f >= 0; f--) {
        double v[6], xn[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double t = s.c[f][i];
#pragma unroll
            for (int p = 0; p < 6; p++) t = fma(-s.O[f][6 * i + p], x[p], t);
            v[i] = t;
        }
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < 6; p++) t = fma(s.inv[f][6 * i + p], v[p], t);
            xn[i] = t;
        }
#pragma unroll
        for (int i = 0; i < 6; i++) { x[i] = xn[i]; s.dl[f][i] = xn[i]; }
    }
    s.flag = ok ? 0 : 1;
}

// The tail, by wavefront 0 after the fresh assembly at the final point, every lane the same registers as in live_solve:
//   elimination   live_solve at mu = 0 leaves P_f^-1 in s.inv
//   marginal      Lambda' = B - O^T A^-1 O, b' = c - O^T A^-1 a, m' = z_1 + Lambda'^-1 b'   (A = D_0 = P_0, a = b_0, O = O_0)
//   covariance    Sigma_{W-1} = P_{W-1}^-1, Sigma_f = P_f^-1 + G_f Sigma_{f+1} G_f^T, G_f = P_f^-1 O_f
// The motion instances take it inline: no call frame, no scratch.
template <bool BANK, bool MOTION>
__device__ __forceinline__ void live_tail_body(LiveShared &s, LiveTail &tl, double *unc, int W, int do_marginal, int do_cov, double lr, double lt, int lane) {
    live_solve(s, W, 0.0);
    const bool ok = s.flag == 0;
    if (do_marginal) {
        // the J_b half of pair (0, 1) alone (lr, lt: its weights): B = J_b^T L_1 J_b, c = -J_b^T L_1 e_0
        {
            double z0[6], z1[6], row0[ENT_STRIDE], row1[ENT_STRIDE], phi[3], et[3], Ma[9], Mb[9];
            ld6(s.z[0], z0);
            ld6(s.z[1], z1);
            make_ent_row(z0, row0);
            make_ent_row(z1, row1);
            pair_terms<true>(row0, row1, live_rel<BANK, MOTION>(s, 1), phi, et, Ma, Mb);
#pragma unroll
            for (int k = 0; k < 36; k++) tl.B[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
#pragma unroll
                for (int j = 0; j < 3; j++) tl.B[6 * k + j] = lr * (Mb[k] * Mb[j] + Mb[3 + k] * Mb[3 + j] + Mb[6 + k] * Mb[6 + j]);
                tl.B[7 * (3 + k)] = lt;
                tl.cB[k] = -lr * (Mb[k] * phi[0] + Mb[3 + k] * phi[1] + Mb[6 + k] * phi[2]);
                tl.cB[3 + k] = -lt * et[k];
            }
        }
        double T[36], L[6][6], bp[6];
        // T = O^T A^-1
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int k = 0; k < 6; k++) {
                double t = 0.0;
#pragma unroll
                for (int p = 0; p < 6; p++) t = fma(s.O[0][6 * p + i], s.inv[0][6 * p + k], t);
                T[6 * i + k] = t;
            }
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int k = 0; k <= i; k++) {
                double t = 0.0;
#pragma unroll
                for (int p = 0; p < 6; p++) t = fma(T[6 * i + p], s.O[0][6 * p + k], t);
                L[i][k] = tl.B[6 * i + k] - t;
                L[k][i] = L[i][k];
            }
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < 6; p++) t = fma(T[6 * i + p], s.b[0][p], t);
            bp[i] = tl.cB[i] - t;
        }
        // the pivots of Lambda' against the pair's own information (L is consumed); the inverse only of a matrix that passed
        double Lk[36], Li[36], mn[6];
#pragma unroll
        for (int i = 0; i < 36; i++) { Lk[i] = L[i / 6][i % 6]; Li[i] = 0.0; }
        bool keep = ok;   // (ok: A = P_0 is among the elimination's pivots)
#pragma unroll
        for (int p = 0; p < 6; p++) {
            const double d = L[p][p];
            keep = keep && d > LIVE_MARGINAL_PIVOT_REL * tl.B[7 * p];
            const double di = 1.0 / (keep ? d : 1.0);
#pragma unroll
            for (int r = p + 1; r < 6; r++)
#pragma unroll
                for (int c = p + 1; c <= r; c++) L[r][c] = fma(-L[r][p] * di, L[c][p], L[r][c]);
        }
        if (keep) {
            double Lc[6][6];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k < 6; k++) Lc[i][k] = Lk[6 * i + k];
            keep = spd6_inverse(Lc, Li);
        }
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < 6; p++) t = fma(Li[6 * i + p], bp[p], t);
            mn[i] = s.z[1][i] + t;
        }
        // (the prior in tl was read by the assembly; nothing reads it after this point)
#pragma unroll
        for (int i = 0; i < 36; i++) tl.Lm[i] = keep ? Lk[i] : 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) tl.m[i] = keep ? mn[i] : 0.0;
        if (lane < 36) unc[LIVE_UNC_LM + lane] = tl.Lm[lane];
        if (lane < 6) unc[LIVE_UNC_M + lane] = tl.m[lane];
        if (lane == 0) { unc[LIVE_UNC_HAS] = keep ? 1.0 : 0.0; unc[LIVE_UNC_DROP] = keep ? 0.0 : 1.0; }
    } else if (lane == 0) {
        unc[LIVE_UNC_HAS] = 0.0;
        unc[LIVE_UNC_DROP] = 0.0;
    }
    if (do_cov) {
        double Sn[36];
#pragma unroll
        for (int i = 0; i < 36; i++) { Sn[i] = s.inv[W - 1][i]; tl.S[W - 1][i] = ok ? Sn[i] : 0.0; }
        for (int f = W - 2; f >= 0; f--) {
            double G[36], GS[36], Sf[36];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    double t = 0.0;
#pragma unroll
                    for (int p = 0; p < 6; p++) t = fma(s.inv[f][6 * i + p], s.O[f][6 * p + k], t);
                    G[6 * i + k] = t;
                }
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    double t = 0.0;
#pragma unroll
                    for (int p = 0; p < 6; p++) t = fma(G[6 * i + p], Sn[6 * p + k], t);
                    GS[6 * i + k] = t;
                }
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k <= i; k++) {
                    double t = s.inv[f][6 * i + k];
#pragma unroll
                    for (int p = 0; p < 6; p++) t = fma(GS[6 * i + p], G[6 * k + p], t);
                    Sf[6 * i + k] = t;
                    Sf[6 * k + i] = t;
                }
#pragma unroll
            for (int i = 0; i < 36; i++) { Sn[i] = Sf[i]; tl.S[f][i] = ok ? Sf[i] : 0.0; }
        }
        for (int k = lane; k < 36 * W; k += 64) unc[LIVE_UNC_HDR + k] = tl.S[k / 36][k % 36];
        if (lane == 0) unc[LIVE_UNC_VALID] = ok ? 1.0 : 0.0;
    } else if (lane == 0) {
        unc[LIVE_UNC_VALID] = 0.0;
    }
}

// The instances of sections 17 - 24 call it: not inlined, it runs when the LM's registers are dead.  One instance per kernel (BANK), so that each
// has ONE caller and keeps seeing that kernel's LDS objects by their addresses.
template <bool BANK>
__device__ __noinline__ void live_tail(LiveShared &s, LiveTail &tl, double *unc, int W, int do_marginal, int do_cov, double lr, double lt, int lane) {
    live_tail_body<BANK, false>(s, tl, unc, W, do_marginal, do_cov, lr, lt, lane);
}

// One push of one tracker by one workgroup of 256 threads: the kernels below call it.  BANK: s is a LiveBankShared whose cnt and lam the caller has filled (a.cnt, a.lam
// are not read) and the threads have met at a barrier since.  MOTION: s is a LiveMotionShared whose rel the caller has filled (no barrier needed: the
// one below comes first); mot takes the pose of the frame before the newest at the final point.  (The prediction a new frame starts from needs nothing
// here: the host puts it into the slot header, where a caller's start pose would be.)
template <bool TAIL, bool BANK, bool MOTION = false>
__device__ __forceinline__ void live_push_body(const LiveArgs &a, LiveShared &s, LiveTail *tl, double *mot = nullptr) {
    const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);   // wave-uniform
    const int W = a.W;
    TrackArgs ta;
    ta.idx = nullptr; ta.uv = nullptr; ta.ent = a.ent; ta.Kmat = a.Kmat; ta.frame_obs_start = nullptr;
    ta.kstride = 9; ta.A = 0; ta.F = W; ta.huber = a.huber; ta.h = a.h;
    ta.max_iters = 0; ta.min_error = ta.min_step_error_diff = ta.min_average_step_error_diff = ta.tau = 0.0;
    ta.z = nullptr; ta.iters_out = nullptr; ta.err_out = nullptr;
    // the window's poses.  The new frame takes the ring slot of the frame that leaves the window: that pose becomes the anchor before the
    // slot is overwritten; the new frame starts from its header's pose or from the previous frame's estimate (read before any write)
    {
        int ns = a.first_slot + W - 1, ps = a.first_slot + W - 2;
        if (ns >= a.slots) ns -= a.slots;
        if (ps >= a.slots) ps -= a.slots;
        if (ps < 0) ps = ns;   // a window of one frame: the previous frame is the one that leaves
        if (t < 6) {
            if (a.has_anchor) {
                const double av = a.zslot[6 * ns + t];
                s.za[t] = av;
                a.anchor[t] = av;
            }
            s.z[W - 1][t] = a.has_init ? reinterpret_cast<const double *>(a.ring + (size_t)ns * a.slot_bytes)[t] : a.zslot[6 * ps + t];
        } else if (t >= 64 && t < 64 + 6 * (W - 1)) {
            const int i = (t - 64) / 6, k = (t - 64) % 6;
            int sl = a.first_slot + i;
            if (sl >= a.slots) sl -= a.slots;
            s.z[i][k] = a.zslot[6 * sl + k];
        }
        if constexpr (TAIL) {
            if (a.marginal && a.has_marginal && t >= 192 && t < 192 + 42) {
                if (t < 192 + 36) tl->Lm[t - 192] = a.unc[LIVE_UNC_LM + t - 192];
                else tl->m[t - 228] = a.unc[LIVE_UNC_M + t - 228];
            }
        }
    }
    __syncthreads();
    bool prior = false;   // the marginal prior is on the first window frame (tail instance only)
    if constexpr (TAIL) prior = a.marginal && a.has_marginal && wv == 0;
    live_eval<true, BANK, MOTION>(a, ta, s, wv, lane);   // init: the first evaluation also yields the first step's system
    if constexpr (TAIL) { if (prior) live_prior<true>(s, *tl, lane); }
    __syncthreads();
    double currData = 0.0, currPrior = 0.0;
    for (int i = 0; i < W; i++) { currData += s.Ef[0][i]; currPrior += s.Pe[0][i]; }
    double currErr = currData + currPrior, prevErr = currErr;
    const double initial = currErr, rows = a.rows;
    double mu = -1.0, v = 2.0;
    int mustExit = 0, iters = 0, rejected = 0, tries = 0;
    for (int it = 0; it < a.max_iters && !mustExit && rows > 0; it++) {
        if (it > 0) {
            live_eval<true, BANK, MOTION>(a, ta, s, wv, lane);   // H, b at the current point (its costs are those already held)
            if constexpr (TAIL) { if (prior) live_prior<true>(s, *tl, lane); }
            __syncthreads();
        }
        if (mu < 0) {
            double mx = s.D[0][0];
            for (int i = 0; i < W; i++)
#pragma unroll
                for (int k = 0; k < 6; k++) mx = fmax(mx, s.D[i][7 * k]);
            mu = mx * a.tau;
        }
        double gain = 0.0;
        int ntries = 0;
        bool accepted = false;
        do {
            if (wv == 0) live_solve(s, W, mu);
            __syncthreads();
            live_eval<false, BANK, MOTION>(a, ta, s, wv, lane);
            if constexpr (TAIL) { if (prior) live_prior<false>(s, *tl, lane); }
            __syncthreads();
            double eD = 0.0, eP = 0.0, d2 = 0.0, dg = 0.0;
            for (int i = 0; i < W; i++) { eD += s.Ef[1][i]; eP += s.Pe[1][i]; d2 += s.lin[i][0]; dg += s.lin[i][1]; }
            const double err = eD + eP;
            const bool bad_pivot = a.smooth && s.flag != 0;   // (track() ignores the pivots of its 6x6 solve)
            const double Lq = 0.5 * (mu * d2 - dg);
            gain = (err - prevErr) / Lq;
            tries++;
            if (!bad_pivot && gain > 0 && (err - prevErr) < 0) {
                const double q = 2 * gain - 1;
                mu = mu * fmax(0.33, 1.0 - q * q * q);
                v = 2.0;
                currErr = err; currData = eD; currPrior = eP;
                if (t < 6 * W) s.z[t / 6][t % 6] = s.zt[t / 6][t % 6];
                if (t >= 128 && t < 128 + W) { s.Ef[0][t - 128] = s.Ef[1][t - 128]; s.Pe[0][t - 128] = s.Pe[1][t - 128]; }
                accepted = true;
            } else {
                if (bad_pivot) gain = 0.0;   // a failed factorisation is a rejected try: more damping, and the retry rule below applies
                mu = mu * v;
                v = v * 5;
                rejected++;
            }
            __syncthreads();   // the decision's reads are done before the next solve or assembly writes
        } while (gain <= 0 && ntries++ < 5 && !accepted);
        if (currErr < a.min_error) mustExit = 1;
        if (fabs(prevErr - currErr) <= a.min_step_error_diff || fabs((prevErr - currErr) / rows) <= a.min_average_step_error_diff || !accepted)
            mustExit = 2;
        if (currErr > prevErr) mustExit = 3;
        iters++;
        prevErr = currErr;
    }
    // the window back into the ring's poses, the costs by window position, the result record
    if (t < 6 * W) {
        int sl = a.first_slot + t / 6;
        if (sl >= a.slots) sl -= a.slots;
        a.zslot[6 * sl + t % 6] = s.z[t / 6][t % 6];
    }
    if (t >= 128 && t < 128 + W) { a.Ef[t - 128] = s.Ef[0][t - 128]; a.Pe[t - 128] = s.Pe[0][t - 128]; }
    if (t >= 192 && t < 198) { a.res[8 + t - 192] = s.z[W - 1][t - 192]; a.res[14 + t - 192] = s.z[0][t - 192]; }
    if constexpr (MOTION) {
        // the frame before the newest: the window's, or with a window of one frame the anchor (zeros before there is one)
        if (t >= 200 && t < 206) mot[t - 200] = W >= 2 ? s.z[W - 2][t - 200] : (a.has_anchor ? s.za[t - 200] : 0.0);
    }
    if (t == 64) {
        a.res[0] = (double)iters; a.res[1] = (double)mustExit; a.res[2] = (double)rejected; a.res[3] = initial;
        a.res[4] = currErr; a.res[5] = currData; a.res[6] = currPrior; a.res[7] = mu;
        a.res[20] = (double)tries; a.res[21] = 0.0; a.res[22] = 0.0; a.res[23] = 0.0;
    }
    if constexpr (TAIL) {
        // one fresh system at the final point, mu = 0, for the marginal of the frame that leaves and for the covariance
        const int do_marginal = a.marginal && W == a.slots, do_cov = a.covariance;
        __syncthreads();   // the stores above have read the costs this assembly writes again
        if (do_marginal || do_cov) {
            live_eval<true, BANK, MOTION>(a, ta, s, wv, lane);
            if (prior) live_prior<true>(s, *tl, lane);
            __syncthreads();
            if (wv == 0) {
                // the motion instances take the tail inline: no call frame, no scratch
                if constexpr (MOTION) live_tail_body<BANK, true>(s, *tl, a.unc, W, do_marginal, do_cov, live_lam<BANK>(a, s, 1, 0), live_lam<BANK>(a, s, 1, 1), lane);
                else live_tail<BANK>(s, *tl, a.unc, W, do_marginal, do_cov, live_lam<BANK>(a, s, 1, 0), live_lam<BANK>(a, s, 1, 1), lane);
            }
        } else if (t < 3) {
            a.unc[t] = 0.0;   // LIVE_UNC_VALID, _HAS, _DROP: the window is still filling
        }
    }
}

template <bool TAIL>
__global__ void __launch_bounds__(256) k_live_push(const LiveArgs a) {
    __shared__ LiveShared s;
    LiveTail *tl = nullptr;
    if constexpr (TAIL) {
        __shared__ LiveTail tail;
        tl = &tail;
    }
    live_push_body<TAIL, false>(a, s, tl);
}

// The constant-velocity instance: k_live_push with an expected motion on every pair, measured by the host when the pair's
// second frame was pushed and carried in the kernel arguments.
template <bool TAIL>
__global__ void __launch_bounds__(256) k_live_push_cv(const LiveMotionArgs ma) {
    __shared__ LiveMotionShared s;
    LiveTail *tl = nullptr;
    if constexpr (TAIL) {
        __shared__ LiveTail tail;
        tl = &tail;
    }
    const int t = threadIdx.x;
    if (t < 6 * ma.a.W) s.rel[t / 6][t % 6] = ma.rel[t / 6][t % 6];
    live_push_body<TAIL, false, true>(ma.a, s, tl, ma.mot);
}

// The bank: workgroup b is member b.  Its LiveArgs: the shared block, the member's row of the table and, from the device's
// own memory, what differs by member and push -- the window's detection counts and whether the new frame brings a start pose (slot headers),
// whether a marginal prior exists (the member's uncertainty record), rows.  Everything is indexed by blockIdx.x alone, hence wave-uniform; the
// workgroups of a launch share nothing but read-only tables.
template <bool TAIL, bool MOTION = false>
__device__ __forceinline__ void live_member_body(const LiveBankArgs &ba, LiveBankShared &s, LiveTail *tl, double *mot = nullptr) {
    const int t = threadIdx.x;
    const LiveMember *m = ba.tab + blockIdx.x;
    LiveArgs a;
    a.ent = uni_ptr(m->ent); a.Kmat = uni_ptr(m->Kmat); a.h = uni_f64(m->h); a.ring = uni_ptr(m->ring);
    a.zslot = uni_ptr(m->zslot); a.anchor = uni_ptr(m->anchor); a.Ef = uni_ptr(m->Ef); a.Pe = uni_ptr(m->Pe);
    a.res = uni_ptr(m->res); a.unc = uni_ptr(m->unc);
    a.slot_bytes = ba.sh.slot_bytes; a.huber = ba.sh.huber;
    a.max_iters = ba.sh.max_iters; a.min_error = ba.sh.min_error; a.min_step_error_diff = ba.sh.min_step_error_diff;
    a.min_average_step_error_diff = ba.sh.min_average_step_error_diff; a.tau = ba.sh.tau;
    a.W = ba.sh.W; a.slots = ba.sh.slots; a.first_slot = ba.sh.first_slot;
    a.has_anchor = ba.sh.has_anchor; a.smooth = ba.sh.smooth; a.anchor_pair = ba.sh.anchor_pair;
    a.marginal = ba.sh.marginal; a.covariance = ba.sh.covariance;
    const int W = a.W;
    if (t < W) s.cnt[t] = (int)reinterpret_cast<const double *>(live_slot(a, t))[LIVE_HDR_CNT];
    if (t >= 64 && t < 64 + 2 * W) s.lam[(t - 64) >> 1][(t - 64) & 1] = ba.sh.lam[(t - 64) >> 1][(t - 64) & 1];
    const double *newest = reinterpret_cast<const double *>(live_slot(a, W - 1));
    a.has_init = ba.raw ? 1 : __builtin_amdgcn_readfirstlane((int)newest[LIVE_HDR_INIT]);
    a.has_marginal = 0;
    if constexpr (TAIL) {
        if (a.marginal && !ba.fresh) a.has_marginal = __builtin_amdgcn_readfirstlane(a.unc[LIVE_UNC_HAS] != 0.0 ? 1 : 0);
    }
    __syncthreads();
    // rows as the host counts them for a single tracker: 8 per detection of the window, 6 per pair, the anchor pair's 6 the marginal prior's
    int det = 0;
    for (int i = 0; i < W; i++) det += live_cnt<true>(a, s, i);
    const int pairs = a.smooth ? W - 1 + (a.marginal ? a.has_marginal : a.has_anchor) : 0;
    a.rows = 8.0 * (double)det + 6.0 * (double)pairs;
    live_push_body<TAIL, true, MOTION>(a, s, tl, mot);
}

template <bool TAIL>
__global__ void __launch_bounds__(256) k_live_push_bank(const LiveBankArgs ba) {
    __shared__ LiveBankShared s;
    LiveTail *tl = nullptr;
    if constexpr (TAIL) {
        __shared__ LiveTail tail;
        tl = &tail;
    }
    live_member_body<TAIL>(ba, s, tl);
}

// The gated single tracker with the motion model: the bank's instance on its one-row table (ONE workgroup), the expected motions in the arguments
// as in k_live_push_cv.
template <bool TAIL>
__global__ void __launch_bounds__(256) k_live_push_member_cv(const LiveMemberMotionArgs ga) {
    __shared__ LiveBankMotionShared s;
    LiveTail *tl = nullptr;
    if constexpr (TAIL) {
        __shared__ LiveTail tail;
        tl = &tail;
    }
    const int t = threadIdx.x;
    if (t >= 128 && t < 128 + 6 * ga.ba.sh.W) s.rel[(t - 128) / 6][(t - 128) % 6] = ga.rel[(t - 128) / 6][(t - 128) % 6];
    live_member_body<TAIL, true>(ga.ba, s, tl, ga.mot);
}

// The bank with the motion model: member b's expected motions lie behind the members' slots of every ring slot, [B][6] doubles at rel_off, and
// came in with the frame that ends the pair (the bank's one copy); they are read where lam is, into LDS by window position.
template <bool TAIL>
__global__ void __launch_bounds__(256) k_live_push_bank_cv(const LiveBankMotionArgs ga) {
    __shared__ LiveBankMotionShared s;
    LiveTail *tl = nullptr;
    if constexpr (TAIL) {
        __shared__ LiveTail tail;
        tl = &tail;
    }
    const int t = threadIdx.x;
    if (t >= 128 && t < 128 + 6 * ga.ba.sh.W) {
        const int i = (t - 128) / 6;
        int sl = ga.ba.sh.first_slot + i;
        if (sl >= ga.ba.sh.slots) sl -= ga.ba.sh.slots;
        s.rel[i][(t - 128) % 6] = reinterpret_cast<const double *>(ga.ring + (size_t)sl * ga.ba.sh.slot_bytes + ga.rel_off)[6 * blockIdx.x + (t - 128) % 6];
    }
    live_member_body<TAIL, true>(ga.ba, s, tl, ga.mot + LIVE_MOT_DOUBLES * blockIdx.x);
}

}  // namespace

void launch_live_push_bank_motion(const LiveBankMotionArgs &a, int B, hipStream_t st) {
    if (a.ba.sh.marginal || a.ba.sh.covariance) hipLaunchKernelGGL(k_live_push_bank_cv<true>, dim3(B), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_live_push_bank_cv<false>, dim3(B), dim3(256), 0, st, a);
}

void launch_live_push_bank(const LiveBankArgs &a, int B, hipStream_t st) {
    if (a.sh.marginal || a.sh.covariance) hipLaunchKernelGGL(k_live_push_bank<true>, dim3(B), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_live_push_bank<false>, dim3(B), dim3(256), 0, st, a);
}

void launch_live_push_member_motion(const LiveMemberMotionArgs &a, hipStream_t st) {
    if (a.ba.sh.marginal || a.ba.sh.covariance) hipLaunchKernelGGL(k_live_push_member_cv<true>, dim3(1), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_live_push_member_cv<false>, dim3(1), dim3(256), 0, st, a);
}

void launch_live_push_motion(const LiveMotionArgs &a, hipStream_t st) {
    if (a.a.marginal || a.a.covariance) hipLaunchKernelGGL(k_live_push_cv<true>, dim3(1), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_live_push_cv<false>, dim3(1), dim3(256), 0, st, a);
}

void launch_live_push(const LiveArgs &a, hipStream_t st) {
    if (a.marginal || a.covariance) hipLaunchKernelGGL(k_live_push<true>, dim3(1), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_live_push<false>, dim3(1), dim3(256), 0, st, a);
}

}  // namespace aar
