#!/bin/bash
# Measurement builds of librvll.so with compile-time switches (A/B on one box): evidence_amd/diag/librvll_<name>.so,
# selected at run time with RVLL_LIBRARY=<path>.  Usage: scripts/build_variants.sh name "-DFLAG ..." [name2 "-D..."] ...
set -e
cd "$(dirname "$0")/../evidence_amd/csrc"
mkdir -p ../diag ../../build/var
FLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -fvisibility=hidden -Wall -Wno-unused-function -I../../include -I."
while [ $# -ge 2 ]; do
  name=$1; defs=$2; shift 2
  B=../../build/var/$name; mkdir -p $B
  /opt/rocm/bin/hipcc $FLAGS $defs -c rvll_kernels.hip -o $B/rvll_kernels.o &
  /opt/rocm/bin/hipcc $FLAGS $defs -mllvm -disable-machine-licm -c rvll_walk.hip -o $B/rvll_walk.o &
  wait
  # every other object of the Makefile's OBJS as `make` left it in build/obj (run make first; the list is the Makefile's)
  others=""
  for o in rvll_api rvll_batch rvll_walk_host rvll_live_host rvll_comm rvll_walk_stepout rvll_fip rvll_live rvll_rounds_runs rvll_cluster \
           rvll_cluster_host rvll_shrinkage rvll_insertion rvll_adapt rvll_merge_setup rvll_merge rvll_posterior rvll_fip_merged \
           rvll_marginal rvll_region rvll_draws rvll_bands rvll_gls rvll_pointwise rvll_prior_density rvll_celerite rvll_celerite_predict; do others="$others ../../build/obj/$o.o"; done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o ../diag/librvll_$name.so $others $B/rvll_kernels.o $B/rvll_walk.o -ldl
  echo "built evidence_amd/diag/librvll_$name.so ($defs)"
done
