// Host side of the HOD rejection filter: the guard flags (make_filter), the envelope table over the mass bins and the staged
// environment / rank ranges (make_cheap), the threshold codes of the 16-bit key filter (make_keytab) and the per-object key
// itself (k16_key, what the hod_build_keys kernel stores).  The filter must never reject an object the reference keeps.
//
// Compiled by hipcc into hod.hip and by g++ into tests/native/envelope_host.cpp, so that the bound is checked on the CPU
// against the oracle's keep masks at parameter and catalogue corners (tests/test_hod_envelope.py).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "../../include/abacus_hip.h"
#include "hod_classify.hpp"

#if defined(__HIPCC__)
#define ENV_HD __host__ __device__ __forceinline__
#else
#define ENV_HD static inline
#endif

namespace abacus_env {

using abacus_cls::SatPre;

// guard flags and float32 constants of the arithmetic bounds (cent_reject / sat_reject in hod.hip)
struct Filt {
    int cent_ok, sat_ok;   // sat_ok: the arithmetic satellite bound applies (particle-independent M1 / M_cut)
    int sat_basic, pad_;   // finite parameters, alpha >= 0, A_s >= 0, ic >= 0 (what the envelope table needs)
    float L_lc, L_Ac, L_Bc, L_inv_s, L_ic;                      // centrals + LRG satellites share lc, sigma
    float E_lc, E_Ac, E_Bc, E_Cc, E_c_phi, E_half_inv_s2, E_ic;  // c_phi = max(2(pmax-1/Q),0) * 0.39894/sigma
    float E_gs;                                                  // gamma / sigma / sqrt(2)
    float Q_lc, Q_Ac, Q_Bc, Q_inv_s, Q_ic;
    // satellites (only used when the tracer's 10**x values are particle independent, SatPre::*_const)
    float L_invM1, L_alpha, L_s[4];
    float E_invM1[3], E_alpha[3], E_As, E_s[4];                  // [default, cent is LRG (EL), cent is ELG (EE)]
    float Q_invM1, Q_alpha, Q_s[4];
    double L_kMcut, E_kMcut, Q_kMcut;                            // kappa * M_cut
};

struct ColRange {
    double lo = 0, hi = 0;
};
struct HodRanges {
    ColRange hdeltac, hfenv, hshear, pdeltac, pfenv, pshear, pranks[4];
};

// mass bins of the envelope table (cheap_bound in hod.hip) and the table itself
constexpr int CH_SHIFT = 20, CH_BASE = (127 + 33) << 3, CH_NLEV = 21 * 8;
struct Cheap {
    int c_ok, s_ok;
    float dec_max;            // >= 1 + sum_q |s_q| |rank_q| for every wanted tracer and every staged rank value
    float pad_;
    float Bc[CH_NLEV], Bs[CH_NLEV];
};

// ---- packed filter keys: 2 bytes per object -------------------------------------------------------------------------------
// The filter compares `random > B[bin(mass)] * weight * dec`.  Everything on the object's side of that inequality is fixed
// once the catalogue and its randoms are staged, so it is folded into ONE 16-bit key per object:
//   low 7 bits   the mass bin: the float32-representation bins of cheap_bound (8 per octave), window 2^36 ... 2^51.9 - bin 0
//                also takes every smaller mass (its bound is the largest of the levels it covers), bin 127 everything above
//                and whatever is not a mass (never rejected);
//   high 9 bits  a CODE of q <= random / weight: exponent and three mantissa bits of the float32 lower bound (its bits >> 20,
//                offset so that code 0 is 2^-44 and below), i.e. q rounded down to eight steps per octave over 2^-44 ... 2^20.
//                `code > code(B[bin] * dec)` implies `random > B[bin] * weight * dec`.  Code 0 is never rejected and also
//                stands for "the division says nothing" (weight < 0 or NaN, random <= 0 or NaN): a bin whose bound lies below
//                2^-44 sends the objects with a random / weight below that (float32 randoms: the zeros) to hod_exact.  Above
//                2^20 codes and bounds saturate at 511: never rejected either; +inf (weight = 0 and a positive random: the
//                marker is 0 * n = 0, never kept) too.
// The coarse q costs candidates - objects whose q lies within a step (6 - 12 %) above the bound - and halves what the filter
// streams: 2 B per object (40 MB at 1e7 + 1e7; 4-B keys with a 16-bit mantissa: 80 MB; float32 shadow columns: 240 MB), one
// LDS table look-up and one integer compare per object, eight tiles per workgroup so that eight 16-B loads per thread are in
// flight.  (Four steps per octave over 2^-100 ... 2^28: +10 % candidates; sixteen over 2^-24 ... 2^8: the satellites of
// massive hosts, whose bound exceeds 2^8, all pass - 2.3e6 instead of 1.3e6 particles at LRG + ELG + QSO.)  Keys are
// rebuilt (one pass) when the randoms change (reseed / update); the parameters never enter them.
constexpr int K16_LEV0 = (36 - 33) * 8;            // CH level that is key bin 0: upper edge 2^36 * 9/8
constexpr int K16_QSHIFT = 20, K16_QOFF = (127 - 44) << 3;   // (float bits >> 20) of 2^-44
ENV_HD int k16_code(float v) {   // v >= 0 or NaN / inf: monotone, saturating
    unsigned int u;
    memcpy(&u, &v, 4);
    const int c = (int)((u & 0x7fffffffu) >> K16_QSHIFT) - K16_QOFF;
    return c < 0 ? 0 : (c > 511 ? 511 : c);
}
// the key of one object: mass (halo mass / host mass), weight (multiplicity / particle weight) and random as staged
ENV_HD unsigned int k16_key(double m, double w, double r) {
    float mf = (float)m;
    if ((double)mf < m) mf = nextafterf(mf, INFINITY);     // rounded up, like the shadow masses
    unsigned int mu;
    memcpy(&mu, &mf, 4);
    const int j = (int)(mu >> CH_SHIFT) - CH_BASE - K16_LEV0;   // negative / NaN masses: sign bit -> above
    const unsigned int bin = (mu >> 31) || !(mf == mf) ? 127u : (j < 0 ? 0u : (j < 127 ? (unsigned int)j : 127u));
    float q = 0.f;
    if (w > 0.0 && r > 0.0) {
        const double qd = r / w * (1.0 - 1e-6);
        q = (float)qd;
        if ((double)q > qd) q = nextafterf(q, 0.f);
        if (!(q == q)) q = 0.f;
    } else if (w == 0.0 && r > 0.0) {
        q = INFINITY;
    }
    return ((unsigned int)k16_code(q) << 7) | bin;
}

struct KeyTab {   // per key bin: the largest q code that is NOT rejected (host-built from the envelope table, make_keytab)
    unsigned short c[128], s[128];
};

inline SatPre make_pre(const abacus_hod_params *p) {
    // particle-independent 10**x values, with libm's pow (the function the CPU path uses for every particle)
    SatPre pre;
    memset(&pre, 0, sizeof pre);
    pre.L_const = p->L_Acent == 0 && p->L_Asat == 0 && p->L_Bcent == 0 && p->L_Bsat == 0;
    pre.E_const = p->E_Acent == 0 && p->E_Asat == 0 && p->E_Bcent == 0 && p->E_Bsat == 0 && p->E_Ccent == 0 &&
                  p->E_Csat == 0;
    pre.Q_const = p->Q_Acent == 0 && p->Q_Asat == 0 && p->Q_Bcent == 0 && p->Q_Bsat == 0;
    pre.L_M1 = pow(10.0, p->L_logM1), pre.L_Mcut = pow(10.0, p->L_logM_cut);
    pre.E_M1 = pow(10.0, p->E_logM1), pre.E_Mcut = pow(10.0, p->E_logM_cut);
    pre.E_M1_EL = pow(10.0, p->E_logM1_EL), pre.E_M1_EE = pow(10.0, p->E_logM1_EE);
    pre.Q_M1 = pow(10.0, p->Q_logM1), pre.Q_Mcut = pow(10.0, p->Q_logM_cut);
    return pre;
}

// host side of the float32 rejection filter: constants rounded so that every bound stays an upper bound
inline Filt make_filter(const abacus_hod_params &p, const SatPre &pre) {
    Filt F;
    memset(&F, 0, sizeof F);
    auto up = [](double v) { return (float)(v * (v >= 0 ? 1.000001 : 0.999999)); };   // >= v after rounding
    auto finite = [](double v) { return std::isfinite(v); };
    bool ok = true;
    auto tracer = [&](bool want, double lc, double Ac, double Bc, double Cc, double sigma, double ic) {
        if (!want) return;
        ok = ok && finite(lc) && finite(Ac) && finite(Bc) && finite(Cc) && finite(sigma) && sigma > 1e-3 && finite(ic) &&
             ic >= 0;
    };
    tracer(p.want_LRG, p.L_logM_cut, p.L_Acent, p.L_Bcent, 0, p.L_sigma, p.L_ic);
    tracer(p.want_ELG, p.E_logM_cut, p.E_Acent, p.E_Bcent, p.E_Ccent, p.E_sigma, p.E_ic);
    tracer(p.want_QSO, p.Q_logM_cut, p.Q_Acent, p.Q_Bcent, 0, p.Q_sigma, p.Q_ic);
    if (p.want_ELG) ok = ok && finite(p.E_p_max) && finite(p.E_Q) && p.E_Q != 0 && finite(p.E_gamma);
    F.cent_ok = ok;
    F.L_lc = (float)p.L_logM_cut, F.L_Ac = (float)p.L_Acent, F.L_Bc = (float)p.L_Bcent;
    F.L_inv_s = (float)(1.0 / (1.41421356 * p.L_sigma)), F.L_ic = up(p.L_ic);
    F.E_lc = (float)p.E_logM_cut, F.E_Ac = (float)p.E_Acent, F.E_Bc = (float)p.E_Bcent, F.E_Cc = (float)p.E_Ccent;
    F.E_c_phi = up(std::max(2.0 * (p.E_p_max - 1.0 / p.E_Q), 0.0) * 0.3989422804014327 / p.E_sigma);
    F.E_half_inv_s2 = (float)(0.5 / (p.E_sigma * p.E_sigma)), F.E_ic = up(p.E_ic);
    F.E_gs = (float)(p.E_gamma / p.E_sigma / 1.4142135623730951);
    F.Q_lc = (float)p.Q_logM_cut, F.Q_Ac = (float)p.Q_Acent, F.Q_Bc = (float)p.Q_Bcent;
    F.Q_inv_s = (float)(1.0 / (1.41421356 * p.Q_sigma)), F.Q_ic = up(p.Q_ic);
    // satellites: the arithmetic bound only when every wanted tracer has particle-independent M1 / M_cut (`sok`); the
    // envelope table of the two-stage filter needs just finite parameters, positive masses and alpha >= 0 (`sbasic`)
    bool sok = ok, sbasic = ok;
    auto sat = [&](bool want, int is_const, double M1, double alpha, double kappa, double Mcut) {
        if (!want) return;
        const bool b = finite(M1) && M1 > 0 && finite(alpha) && alpha >= 0 && finite(kappa) && finite(Mcut);
        sbasic = sbasic && b;
        sok = sok && is_const && b;
    };
    sat(p.want_LRG, pre.L_const, pre.L_M1, p.L_alpha, p.L_kappa, pre.L_Mcut);
    sat(p.want_ELG, pre.E_const, pre.E_M1, p.E_alpha, p.E_kappa, pre.E_Mcut);
    sat(p.want_ELG, pre.E_const, pre.E_M1_EL, p.E_alpha_EL, p.E_kappa, pre.E_Mcut);
    sat(p.want_ELG, pre.E_const, pre.E_M1_EE, p.E_alpha_EE, p.E_kappa, pre.E_Mcut);
    sat(p.want_QSO, pre.Q_const, pre.Q_M1, p.Q_alpha, p.Q_kappa, pre.Q_Mcut);
    if (p.want_ELG) sok = sok && finite(p.E_A_s) && p.E_A_s >= 0, sbasic = sbasic && finite(p.E_A_s) && p.E_A_s >= 0;
    F.sat_ok = sok;
    F.sat_basic = sbasic;
    F.L_invM1 = up(1.0 / pre.L_M1), F.L_alpha = (float)p.L_alpha;
    F.E_invM1[0] = up(1.0 / pre.E_M1), F.E_invM1[1] = up(1.0 / pre.E_M1_EL), F.E_invM1[2] = up(1.0 / pre.E_M1_EE);
    F.E_alpha[0] = (float)p.E_alpha, F.E_alpha[1] = (float)p.E_alpha_EL, F.E_alpha[2] = (float)p.E_alpha_EE;
    F.E_As = up(p.E_A_s);
    F.Q_invM1 = up(1.0 / pre.Q_M1), F.Q_alpha = (float)p.Q_alpha;
    const double Ls[4] = {p.L_s, p.L_s_v, p.L_s_p, p.L_s_r}, Es[4] = {p.E_s, p.E_s_v, p.E_s_p, p.E_s_r},
                 Qs[4] = {p.Q_s, p.Q_s_v, p.Q_s_p, p.Q_s_r};
    for (int q = 0; q < 4; q++) {
        F.L_s[q] = (float)Ls[q], F.E_s[q] = (float)Es[q], F.Q_s[q] = (float)Qs[q];
        if (p.enable_ranks) {
            const bool b = finite(Ls[q]) && finite(Es[q]) && finite(Qs[q]);
            F.sat_ok = F.sat_ok && b, F.sat_basic = F.sat_basic && b;
        }
    }
    // kappa*M_cut exactly as n_sat_* forms it (FP64 product)
    F.L_kMcut = p.L_kappa * pre.L_Mcut, F.E_kMcut = p.E_kappa * pre.E_Mcut, F.Q_kMcut = p.Q_kappa * pre.Q_Mcut;
    return F;
}

// Value ranges of the staged environment / rank columns (NaNs ignored), measured once per catalogue: the envelope
// table bounds every object's occupation by the occupation at the most favourable environment in these ranges.
inline void prod_range(double c, const ColRange &r, double &lo, double &hi) {   // range of c * x, x in r
    const double a = c * r.lo, b = c * r.hi;
    if (c == 0) return;   // the reference forms 0 * x: exactly 0 for finite x
    lo += std::min(a, b), hi += std::max(a, b);
}

// host side of the two-stage filter: an ENVELOPE table - for every float32 mass bin an upper bound of the summed
// occupation of the wanted tracers over the masses of the bin AND over the staged ranges of deltac / fenv / shear, so the
// streaming loop reads mass, multiplicity / weight and random only (12 B per object) for any HOD:
//   erfc forms (LRG / QSO centrals, the LRG satellites' n_cen factor): largest at the bin's upper edge and the smallest
//   logM_cut + A d + B f of the range;  ELG centrals 2 (p_max - 1/Q) phi(x) Phi(gamma x), x = (logM - logM_cut') / sigma
//   (not monotone): Gaussian at the smallest |logM - logM_cut'| the bin and the range admit, Phi at the largest gamma x;
//   power laws ((M - kappa M_cut') / M1')^alpha: upper edge, smallest kappa M_cut' and smallest M1' of the range, the
//   largest of the three conformity variants for ELG.  Rank modulation: 1 + sum |s_q| max |rank_q|.
inline Cheap make_cheap(const abacus_hod_params &p, const Filt &F, const HodRanges &R, bool one_stage) {
    Cheap c;
    memset(&c, 0, sizeof c);
    c.c_ok = F.cent_ok && (p.want_LRG || p.want_ELG || p.want_QSO) && !one_stage;
    c.s_ok = F.sat_basic && (p.want_LRG || p.want_ELG || p.want_QSO) && !one_stage;
    auto up = [](double v) { return std::max((float)(v * 1.00001), 1e-30f); };
    // ranges of logM_cut' (centrals: halo columns; satellites: particle columns) and of logM1' per tracer / variant
    struct LR {
        double lo, hi;
    };
    auto lin = [&](double base, double A, const ColRange &d, double B, const ColRange &f, double Cc, const ColRange &sh) {
        LR r{base, base};
        prod_range(A, d, r.lo, r.hi), prod_range(B, f, r.lo, r.hi), prod_range(Cc, sh, r.lo, r.hi);
        return r;
    };
    const LR Lc_h = lin(p.L_logM_cut, p.L_Acent, R.hdeltac, p.L_Bcent, R.hfenv, 0, R.hshear);
    const LR Ec_h = lin(p.E_logM_cut, p.E_Acent, R.hdeltac, p.E_Bcent, R.hfenv, p.E_Ccent, R.hshear);
    const LR Qc_h = lin(p.Q_logM_cut, p.Q_Acent, R.hdeltac, p.Q_Bcent, R.hfenv, 0, R.hshear);
    const LR Lc_p = lin(p.L_logM_cut, p.L_Acent, R.pdeltac, p.L_Bcent, R.pfenv, 0, R.pshear);
    const LR Ec_p = lin(p.E_logM_cut, p.E_Acent, R.pdeltac, p.E_Bcent, R.pfenv, p.E_Ccent, R.pshear);
    const LR Qc_p = lin(p.Q_logM_cut, p.Q_Acent, R.pdeltac, p.Q_Bcent, R.pfenv, 0, R.pshear);
    const LR L1 = lin(p.L_logM1, p.L_Asat, R.pdeltac, p.L_Bsat, R.pfenv, 0, R.pshear);
    const LR E1 = lin(p.E_logM1, p.E_Asat, R.pdeltac, p.E_Bsat, R.pfenv, p.E_Csat, R.pshear);
    const LR E1L = lin(p.E_logM1_EL, p.E_Asat, R.pdeltac, p.E_Bsat, R.pfenv, 0, R.pshear);   // no Csat term (:1006-1035)
    const LR E1E = lin(p.E_logM1_EE, p.E_Asat, R.pdeltac, p.E_Bsat, R.pfenv, 0, R.pshear);
    const LR Q1 = lin(p.Q_logM1, p.Q_Asat, R.pdeltac, p.Q_Bsat, R.pfenv, 0, R.pshear);
    double dec = 1.0;
    if (p.enable_ranks) {
        const double Ls[4] = {p.L_s, p.L_s_v, p.L_s_p, p.L_s_r}, Es[4] = {p.E_s, p.E_s_v, p.E_s_p, p.E_s_r},
                     Qs[4] = {p.Q_s, p.Q_s_v, p.Q_s_p, p.Q_s_r};
        for (int q = 0; q < 4; q++) {
            double m = 0;
            if (p.want_LRG) m = std::max(m, std::fabs(Ls[q]));
            if (p.want_ELG) m = std::max(m, std::fabs(Es[q]));
            if (p.want_QSO) m = std::max(m, std::fabs(Qs[q]));
            dec += m * std::max(std::fabs(R.pranks[q].lo), std::fabs(R.pranks[q].hi));
        }
    }
    if (!std::isfinite(dec)) c.s_ok = 0;
    c.dec_max = (float)(dec * 1.0001);
    auto half_erfc = [](double lM, double lc, double sigma) { return 0.5 * std::erfc((lc - lM) / (1.41421356 * sigma)); };
    auto powa = [](double x, double a) { return a == 1.0 ? x : std::pow(x, a); };
    // ((M - kappa M_cut') / M1')^alpha at its largest: smallest kappa * 10^lc and smallest 10^l1 of the ranges.  The two
    // mass-independent factors are evaluated once per call, not per level (their pow() calls were most of this function)
    struct PL {
        double kM, M1, alpha;
    };
    auto plaw_of = [](double kappa, const LR &lc, const LR &l1, double alpha) {
        return PL{std::min(kappa * std::pow(10.0, lc.lo), kappa * std::pow(10.0, lc.hi)), std::pow(10.0, l1.lo), alpha};
    };
    auto plaw = [&](double M, const PL &f) {
        const double x = M - f.kM;
        return x < 0 ? 0.0 : powa(x / f.M1, f.alpha);
    };
    const PL pL = plaw_of(p.L_kappa, Lc_p, L1, p.L_alpha), pE = plaw_of(p.E_kappa, Ec_p, E1, p.E_alpha),
             pEL = plaw_of(p.E_kappa, Ec_p, E1L, p.E_alpha_EL), pEE = plaw_of(p.E_kappa, Ec_p, E1E, p.E_alpha_EE),
             pQ = plaw_of(p.Q_kappa, Qc_p, Q1, p.Q_alpha);
    // upper edges of the bins and their log10: constants of the binning, evaluated once per process
    struct Edges {
        double T[CH_NLEV], lM[CH_NLEV];
    };
    static const Edges edges = [] {
        Edges e;
        for (int j = 0; j < CH_NLEV; j++) {
            const uint32_t bits = (uint32_t)(CH_BASE + j + 1) << CH_SHIFT;   // upper edge of bin j (exclusive)
            float Tf;
            memcpy(&Tf, &bits, 4);
            e.T[j] = (double)Tf, e.lM[j] = std::log10(e.T[j]);
        }
        return e;
    }();
    // without an environment term the LRG centrals and satellites share logM_cut': one erfc per level serves both
    const bool L_same = Lc_h.lo == Lc_p.lo;
    double lM_prev = -INFINITY;   // bin 0 also takes every smaller mass
    for (int j = 0; j < CH_NLEV; j++) {
        const double T = edges.T[j], lM = edges.lM[j];
        double bc = 0, bs = 0, eLc = 0;
        if (c.c_ok) {
            if (p.want_LRG) bc += (eLc = half_erfc(lM, Lc_h.lo, p.L_sigma)) * p.L_ic;
            if (p.want_QSO) bc += half_erfc(lM, Qc_h.lo, p.Q_sigma) * p.Q_ic;   // 0.5 (1 + erf(u)) = 0.5 erfc(-u)
            if (p.want_ELG) {
                // d = logM - logM_cut' over the bin (its lower edge widened by the round-up of the shadow mass) and the range
                const double dl = (lM_prev - 1e-6) - Ec_h.hi, dh = lM - Ec_h.lo;
                const double dmin = (dl <= 0 && dh >= 0) ? 0.0 : std::min(std::fabs(dl), std::fabs(dh));
                const double phi = 0.3989422804014327 / p.E_sigma * std::exp(-(dmin * dmin) / 2 / (p.E_sigma * p.E_sigma));
                const double xmax = std::max(p.E_gamma * dl / p.E_sigma, p.E_gamma * dh / p.E_sigma);
                const double Phi = std::isfinite(xmax) ? 0.5 * (1 + std::erf(xmax / 1.4142135623730951)) : 1.0;
                bc += std::max(2.0 * (p.E_p_max - 1.0 / p.E_Q), 0.0) * phi * Phi * p.E_ic;
            }
        }
        if (c.s_ok) {
            if (p.want_LRG) bs += plaw(T, pL) * (L_same && c.c_ok ? eLc : half_erfc(lM, Lc_p.lo, p.L_sigma)) * p.L_ic;
            if (p.want_ELG) {
                const double v = std::max(plaw(T, pE), std::max(plaw(T, pEL), plaw(T, pEE)));
                bs += p.E_A_s * v * p.E_ic;
            }
            if (p.want_QSO) bs += plaw(T, pQ) * p.Q_ic;
        }
        if (!std::isfinite(bc)) c.c_ok = 0;
        if (!std::isfinite(bs)) c.s_ok = 0;
        c.Bc[j] = up(bc), c.Bs[j] = up(bs);
        lM_prev = lM;
    }
    return c;
}

// threshold codes of the 16-bit key filter from the envelope table (see hod_build_keys): key bin b = table level
// K16_LEV0 + b; bin 0 also covers every level below it, bin 127 is never rejected
inline KeyTab make_keytab(const Cheap &ch) {
    KeyTab kt;
    for (int sat = 0; sat < 2; sat++) {
        const float *B = sat ? ch.Bs : ch.Bc;
        const float dec = sat ? ch.dec_max : 1.0f;   // folded into the table
        for (int b = 0; b < 128; b++) {
            float v = INFINITY;
            if (b == 0) {
                v = 0.f;
                for (int l = 0; l <= K16_LEV0; l++) v = std::fmax(v, B[l]);
            } else if (b < 127 && K16_LEV0 + b < CH_NLEV) {
                v = B[K16_LEV0 + b];
            }
            (sat ? kt.s : kt.c)[b] = (unsigned short)k16_code(v * dec * 1.0001f);   // NaN / inf saturate at 511: never rejected
        }
    }
    return kt;
}

}  // namespace abacus_env
