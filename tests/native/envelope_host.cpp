// Host build of abacusutils_amd/csrc/hod_envelope.hpp (g++): the guard flags, the envelope table, the threshold codes and
// the per-object key of the HOD rejection filter, so that the CPU suite can hold `code(key) <= table[bin(key)]` against the
// oracle's exact keep masks (tests/test_hod_envelope.py).  Test infrastructure only.
#include "../../abacusutils_amd/csrc/hod_envelope.hpp"

using namespace abacus_env;

extern "C" {

// ranges: lo, hi of hdeltac, hfenv, hshear, pdeltac, pfenv, pshear, pranks, pranksv, pranksp, pranksr (20 doubles)
// flags: cent_ok, sat_ok, sat_basic, c_ok, s_ok;  tab_c / tab_s: the 128 threshold codes per kind
void env_tables(const abacus_hod_params *p, const double *ranges, int one_stage, int *flags, float *dec_max,
                unsigned short *tab_c, unsigned short *tab_s) {
    HodRanges R;
    ColRange *r[10] = {&R.hdeltac, &R.hfenv, &R.hshear, &R.pdeltac, &R.pfenv, &R.pshear, &R.pranks[0], &R.pranks[1],
                       &R.pranks[2], &R.pranks[3]};
    for (int i = 0; i < 10; i++) r[i]->lo = ranges[2 * i], r[i]->hi = ranges[2 * i + 1];
    const SatPre pre = make_pre(p);
    const Filt F = make_filter(*p, pre);
    const Cheap ch = make_cheap(*p, F, R, one_stage != 0);
    const KeyTab kt = make_keytab(ch);
    flags[0] = F.cent_ok, flags[1] = F.sat_ok, flags[2] = F.sat_basic, flags[3] = ch.c_ok, flags[4] = ch.s_ok;
    *dec_max = ch.dec_max;
    memcpy(tab_c, kt.c, sizeof kt.c);
    memcpy(tab_s, kt.s, sizeof kt.s);
}

void env_keys(int64_t n, const double *mass, const double *wgt, const double *rnd, unsigned short *keys) {
    for (int64_t i = 0; i < n; i++) keys[i] = (unsigned short)k16_key(mass[i], wgt[i], rnd[i]);
}

}  // extern "C"
