#!/bin/bash
# Experiment build of the headline kernel only (-DUPR_HEADLINE_ONLY: ~45 s instead of 2.5 min) into libupright_mi_exp.so;
# extra -D flags are passed through.  Run with UPR_LIB=libupright_mi_exp.so.  Never the production library.
set -e
cd "$(dirname "$0")/.."
python -c 'import sys; from __graft_entry__ import build_engine; build_engine(out=sys.argv[1], extra_flags=["-DUPR_MONOLITHIC", "-DUPR_HEADLINE_ONLY", *sys.argv[2:]])' \
    "upright_amd/${OUT:-libupright_mi_exp.so}" "$@" 2>&1 | grep -E "error" || true
ls -l upright_amd/${OUT:-libupright_mi_exp.so}
