#!/bin/bash
# Rebuild the units of the C-ABI alone (__graft_entry__.ENGINE_UNITS: C-ABI, balance family, linearisation and line search, generic
# QP kernels) and relink libupright_mi.so with the production QP kernel's objects as they are (upright_amd/csrc/build/upr_qp3_part*.o;
# a full __graft_entry__.build_engine() makes all).  Extra compiler flags are passed through.
set -e
cd "$(dirname "$0")/.."
python -c 'import sys; from __graft_entry__ import build_engine; build_engine(extra_flags=sys.argv[1:], qp3_parts=False)' "$@" 2>&1 | grep -E "error" || true
