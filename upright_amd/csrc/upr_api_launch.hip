// upr_api_launch.hip -- the linearisation and line-search kernels of libupright_mi.so: every instantiation the lists of
// upr_launch_select.h name (upr_linearize.h, upr_linearize2.h, upr_linesearch.h) and their launches.
// What crosses to upr_api.hip (upr_handle.h): upr_launch_resolve, the part of upr_batch_create that plans the two kernels of a
// handle from the problem and the knobs and resolves the plan to an instantiation, and launch_linearize / launch_linesearch.
// The phase counters of the instrumented builds (-DUPR_LIN_PROF, -DUPR_LS_PROF) live here, with the entries that read them.
#define UPR_UNIT_LAUNCH
#include "upr_handle.h"

namespace {

// the instantiation a choice names, at the handle's chain length: the lists of upr_launch_select.h expanded
template <int NQ>
const void* lin_kernel(const upr_lin_choice& s) {
    if (s.kind == 2) return (const void*)upr_linearize2_kernel<NQ>;
#define X(M, O, R, NP) if (s.mfma == M && s.occ == O && s.ori == R && s.npass == NP) return (const void*)upr_linearize_kernel<NQ, M, O, R, NP>;
    UPR_LIN_FORMS(X)
#undef X
    return nullptr;
}
template <int NQ>
void (*ls_kernel(const upr_ls_choice& s))(upr_ls_args) {
    // (STAGE is compile-time in the kernel: its staged arrays are LDS pointers, not generic ones)
#define X(NF, NB, E, O) if (s.nfm == NF && s.nbm == NB && s.exact == E && s.obs == O) \
        return s.stage ? upr_linesearch_kernel<NQ, 128, NF, NB, E, O, true> : upr_linesearch_kernel<NQ, 128, NF, NB, E, O, false>;
    UPR_LS_FORMS(X)
#undef X
    return nullptr;
}

}  // namespace

// the linearisation and line-search kernels of a handle (upr_launch_select.h), resolved once at upr_batch_create
int upr_launch_resolve(upr_batch* h) {
    const upr_problem* P = &h->P;
    const upr_dims& d = h->d;
    upr_lin_knobs kl; upr_ls_knobs ks;
    if (const char* e = getenv("UPR_LIN_MFMA")) kl.mfma = atoi(e) != 0;
    if (const char* e = getenv("UPR_LIN2")) kl.lin2 = atoi(e) != 0;
    if (const char* e = getenv("UPR_LIN_OCC")) kl.occ = atoi(e);
    if (const char* e = getenv("UPR_LIN_ROW_PASSES")) kl.row_passes = atoi(e);
    if (const char* e = getenv("UPR_LS_STAGE_FULL")) ks.stage_full = atoi(e);
    static_cast<upr_lin_choice&>(h->lin_sel) = upr_lin_plan(*P, d, kl);
    static_cast<upr_ls_choice&>(h->ls_sel) = upr_ls_plan(*P, d, ks);
    h->lin_sel.kern = (P->nq == 6) ? lin_kernel<6>(h->lin_sel) : lin_kernel<9>(h->lin_sel);
    h->ls_sel.kern = (P->nq == 6) ? ls_kernel<6>(h->ls_sel) : ls_kernel<9>(h->ls_sel);
    upr_ls_name(h->ls_sel, h->ls_sel.name, sizeof(h->ls_sel.name));
    if (!h->lin_sel.kern || !h->ls_sel.kern) return upr_fail("the planned linearisation / line-search form is not an instantiation of upr_launch_select.h's lists");
    return 0;
}

// the linearisation kernel of the handle (lin_sel) over A.npoints knots
int launch_linearize(upr_batch* h, const upr_lin_args& A) {
    const upr_lin_sel& s = h->lin_sel;
    if (s.too_large) return upr_fail("collision model too large for the linearisation kernel's LDS");
    if (s.lds > 64 * 1024) UPR_HIP(hipFuncSetAttribute(s.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds));
    const int blocks = (A.npoints + s.kpw - 1) / s.kpw;
    upr_lin_args Ac = A;
    int kpw = s.kpw, n_sph = h->P.n_sph;
    void* args[] = {&Ac, &kpw, &n_sph};   // (a kernel takes as many as it declares: upr_linearize_kernel the first alone)
    UPR_HIP(hipLaunchKernel(s.kern, dim3(blocks), dim3(256), args, s.lds, h->stream));
    h->lin_blocks_last = blocks;
    return 0;
}

// the line-search kernel of the handle (ls_sel), one workgroup per instance
int launch_linesearch(upr_batch* h, const upr_ls_args& A0) {
    const upr_ls_sel& s = h->ls_sel;
    upr_ls_args A = A0;
    A.n_way = h->P.n_way;
    static_assert(3 * UPR_MAX_WAYPOINTS <= 128, "a lane per waypoint coordinate");
    A.stage_full = s.stage ? 1 : 0;
    if (s.lds > 160 * 1024) return upr_fail("horizon too long for the line-search kernel's LDS");
    if (s.lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)s.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds);
    // two waves per instance (wave 0: the chain walks of a trial, wave 1: its flat sums): 241 registers, four workgroups per CU by
    // LDS.  Four waves (more flat lanes, 128 registers a lane for four workgroups per CU: 135 spilled) measured 48 against 33 us.
    hipLaunchKernelGGL(s.kern, dim3(h->B), dim3(128), s.lds, h->stream, A);
    h->ls_launched = true;
    UPR_HIP(hipGetLastError());
    return 0;
}

#ifdef UPR_LS_PROF
// instrumented build only: cycles from the start of the line-search kernel to each of its stamps, summed over workgroups, [15] = workgroups
extern "C" int upr_debug_ls_prof(double* out, int reset) {
    unsigned long long h[16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(upr_ls_prof), sizeof(h)) != hipSuccess) return 1;
    for (int i = 0; i < 16; ++i) out[i] = (double)h[i];
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(upr_ls_prof), z, sizeof(z)) != hipSuccess) return 1; }
    return 0;
}
#endif
#ifdef UPR_LIN_PROF
// instrumented build only: cycles per phase of the linearisation kernel summed over workgroups, [7] = workgroups counted
extern "C" int upr_debug_lin_prof(double* out, int reset) {
    unsigned long long h[8];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(upr_lin_prof), sizeof(h)) != hipSuccess) return 1;
    for (int i = 0; i < 8; ++i) out[i] = (double)h[i];
    if (reset) { unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0}; if (hipMemcpyToSymbol(HIP_SYMBOL(upr_lin_prof), z, sizeof(z)) != hipSuccess) return 1; }
    return 0;
}
#endif
