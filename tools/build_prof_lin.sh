#!/bin/bash
# Instrumented build of the linearisation / line-search kernels (phase stamps: -DUPR_LIN_PROF -DUPR_LS_PROF) into
# upright_amd/libupright_mi_prof.so: the units of the C-ABI alone are recompiled (__graft_entry__.build_engine), the production QP
# kernel's objects are linked as built.
#   tools/build_prof_lin.sh && gpurun -- 'UPR_LIB=libupright_mi_prof.so python tools/dbg_ls.py; UPR_LIB=libupright_mi_prof.so python tools/dbg_lin.py'
set -e
cd "$(dirname "$0")/.."
python -c 'import sys; from __graft_entry__ import build_engine; build_engine(out="upright_amd/libupright_mi_prof.so", extra_flags=["-DUPR_LIN_PROF", "-DUPR_LS_PROF", *sys.argv[1:]], qp3_parts=False)' "$@"
ls -l upright_amd/libupright_mi_prof.so
