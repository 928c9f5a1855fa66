// upr_api_qp_old.hip -- the two older QP structures of libupright_mi.so: every instantiation of the generic kernel (upr_qp.h,
// upr_qp_kernel<NT>) and of the second-structure kernel (upr_qp2.h, upr_qp2_kernel<D, NT> for the UPR_QP2_SHAPES) with its launcher.
// What crosses to upr_api.hip (upr_handle.h): qp_generic_launcher(nt) and qp2_launcher(nq, nb, nc, nf, nt), each the launcher
// that qp_resolve stores in the handle's selection record; where the kernels leave their factors is host layout and stays there.
#include "upr_handle.h"

namespace {

// generic (runtime-dimension) QP kernel, at the workgroup size upr_qp_generic_nt chose
template <int NT>
int launch_qp_generic_nt(upr_batch* h, const upr_qp_args& A) {
    const upr_qp_lds lay = upr_qp_lds_layout(A.d, NT);
    const size_t lds = (size_t)lay.total * sizeof(double);
    if (lds > 160 * 1024) return upr_fail("QP working set exceeds 160 KiB of LDS");
    if (lds > 64 * 1024) UPR_HIP(hipFuncSetAttribute((const void*)upr_qp_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(upr_qp_kernel<NT>, dim3(h->B), dim3(NT), lds, h->stream, A);
    UPR_HIP(hipGetLastError());
    return 0;
}
int launch_qp_generic_bad_nt(upr_batch*, const upr_qp_args&) { return upr_fail("UPR_QP_GENERIC_NT must be 64, 128, 256, 512 or 1024"); }
}  // namespace

upr_qp_launcher qp_generic_launcher(int nt) {
    switch (nt) {
        case 64: return launch_qp_generic_nt<64>;
        case 128: return launch_qp_generic_nt<128>;
        case 256: return launch_qp_generic_nt<256>;
        case 512: return launch_qp_generic_nt<512>;
        case 1024: return launch_qp_generic_nt<1024>;
        default: return launch_qp_generic_bad_nt;
    }
}

namespace {

template <class D, int NT>
int launch_qp2_nt(upr_batch* h, const upr_qp_args& A) {
    const size_t lds = upr_qp2_lds_doubles<D>(A.d.N, NT) * sizeof(double);
    if (lds > 160 * 1024) return upr_fail("QP working set exceeds 160 KiB of LDS");
    if (lds > 64 * 1024) UPR_HIP(hipFuncSetAttribute((const void*)upr_qp2_kernel<D, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((upr_qp2_kernel<D, NT>), dim3(h->B), dim3(NT), lds, h->stream, A);
    UPR_HIP(hipGetLastError());
    return 0;
}
int launch_qp2_bad_nt(upr_batch*, const upr_qp_args&) { return upr_fail("UPR_QP_NT must be 64, 128 or 256"); }
template <class D>
upr_qp_launcher qp2_launcher(int nt) {
    switch (nt) {
        case 64: return launch_qp2_nt<D, 64>;
        case 512:
        case 128: return launch_qp2_nt<D, 128>;
        case 256: return launch_qp2_nt<D, 256>;
        default: return launch_qp2_bad_nt;
    }
}
}  // namespace

upr_qp_launcher qp2_launcher(int nq, int nb, int nc, int nf, int nt) {
#define X(a, b, c, e) if (nq == a && nb == b && nc == c && nf == e) return qp2_launcher<upr_qp2_dims<a, b, c, e>>(nt);
    UPR_QP2_SHAPES(X)
#undef X
    return nullptr;
}
