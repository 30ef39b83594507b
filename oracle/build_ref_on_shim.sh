#!/bin/bash
# Build container only: compiles the reference's LinearElasticity.cc / Filter.cc / PDEFilter.cc IN PLACE (unchanged,
# from the reference checkout) against include/petsc_compat and links them, with host/ref_driver.cc, against the shim.
# Output: oracle/_ref/ref_on_shim, oracle/_ref/topopt_ref (the reference's whole program) and oracle/_ref/ref_mma,
# git-ignored; they travel with the working tree to a GPU box that has no reference checkout.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REF=${REFERENCE_DIR:-/root/reference}
[ -d "$REF" ] || { echo "no reference sources at $REF"; exit 3; }
OUT=$ROOT/oracle/_ref
LIB=$ROOT/topopt_in_petsc_amd
COMPAT=$ROOT/include/petsc_compat
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir -p "$OUT"
make -s -C "$ROOT/host" ../topopt_in_petsc_amd/libtopopt_petsc_shim.so
# (rpath: oracle/_ref/../../topopt_in_petsc_amd)
LINK=(-L"$LIB" -ltopopt_petsc_shim -ltopopt_amd -Wl,-rpath,'$ORIGIN/../../topopt_in_petsc_amd' -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib)
for f in LinearElasticity Filter PDEFilter; do
  g++ -std=c++11 -O2 -w -I"$COMPAT" -I"$REF" -c "$REF/$f.cc" -o "$TMP/$f.o"
done
g++ -std=c++11 -O2 -w -I"$COMPAT" -I"$REF" -c "$ROOT/host/ref_driver.cc" -o "$TMP/driver.o"
g++ -o "$OUT/ref_on_shim" "$TMP"/driver.o "$TMP"/LinearElasticity.o "$TMP"/Filter.o "$TMP"/PDEFilter.o "${LINK[@]}"
# the WHOLE reference program, all eight sources unchanged (main.cc, TopOpt.cc, MMA.cc, MPIIO.cc + the three above)
for f in main TopOpt MMA MPIIO; do
  g++ -std=c++11 -O2 -w -I"$COMPAT" -I"$REF" -c "$REF/$f.cc" -o "$TMP/$f.o"
done
g++ -o "$OUT/topopt_ref" "$TMP"/main.o "$TMP"/TopOpt.o "$TMP"/MMA.o "$TMP"/MPIIO.o "$TMP"/LinearElasticity.o "$TMP"/Filter.o "$TMP"/PDEFilter.o "${LINK[@]}"
# the reference's MMA class alone, around host/ref_mma_driver.cc (m > 1 constraints)
g++ -std=c++11 -O2 -w -I"$COMPAT" -I"$REF" -c "$ROOT/host/ref_mma_driver.cc" -o "$TMP/mma_driver.o"
g++ -o "$OUT/ref_mma" "$TMP"/mma_driver.o "$TMP"/MMA.o "${LINK[@]}"
echo "built $OUT/ref_on_shim $OUT/topopt_ref $OUT/ref_mma"
