// upr_bal_dims.h -- the layout of one job of the balance family (upr_balance.h).  On its own so that the handle (upr_handle.h) can
// hold one without the family's kernels: those are defined in upr_api_balance.hip alone.
#pragma once
#include "upr_common.h"

struct upr_bal_dims {
    int m, ncol, gpc, mp;   // rows 6 nb, columns, generators per contact (4 | 1), largest passive set min(m, ncol)
    // workspace of one job (doubles): b, r [m]; zp, s, y, dg [mp]; passive columns [mp][12]; normal matrix / factor [mp][mp];
    // then ints: column of every passive slot [mp], its two bodies [mp][2], state of every column [ncol] (0 free, 1 passive, 2 barred)
    int o_b, o_r, o_zp, o_s, o_y, o_dg, o_pcol, o_G, o_int, total;
};
static inline UPR_HD upr_bal_dims upr_bal_layout(int nb, int nc, int nf) {
    upr_bal_dims L;
    L.m = 6 * nb; L.gpc = (nf == 3) ? 4 : 1; L.ncol = L.gpc * nc; L.mp = L.m < L.ncol ? L.m : L.ncol;
    L.o_b = 0; L.o_r = L.o_b + L.m; L.o_zp = L.o_r + L.m; L.o_s = L.o_zp + L.mp; L.o_y = L.o_s + L.mp; L.o_dg = L.o_y + L.mp;
    L.o_pcol = L.o_dg + L.mp; L.o_G = L.o_pcol + 12 * L.mp; L.o_int = L.o_G + L.mp * L.mp;
    L.total = L.o_int + (3 * L.mp + L.ncol + 1) / 2;
    return L;
}
