#!/usr/bin/env bash
# TEST / BENCH DATA: the equilibrium files written by the reference's own solovev_2_eqdsk.  Runs
# oracle/_ref/solovev_2_eqdsk (RAYS_project/solovev_2_eqdsk/solovev_2_eqdsk.f90 compiled from /root/reference by
# oracle/build_ref.sh) on a namelist of configs/ and keeps its output, configs/<eqdsk_file_name of the namelist> (a data
# file: psi(R, Z) on the grid, R B_phi, the boundary).
#
#   oracle/make_cfg5_eqdsk.sh [namelist ...]      default: both of
#     solovev_2_eqdsk_129.in     BASELINE config 5's file as SURVEY 8(d) wrote it -- "eqdsk 129 x 129 written by the
#                                reference's own solovev_2_eqdsk" -- on the Solovev equilibrium of every other config of this
#                                repo (rmaj 1, kappa 1.1, B0 3.3 T, outer boundary 1.4, box 0.5..1.5 x -0.7..0.7)
#     solovev_2_eqdsk_49x65.in   the same equilibrium on the box 0.48..1.56 x -0.74..0.74, 49 x 65 points: grid spacings
#                                that are no powers of two, so that the cell estimate of the spline lookups rounds across
#                                grid lines in R as well as in Z (tests/rhs_state_cases.py: class K)
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/.." && pwd)
BIN=$HERE/_ref/solovev_2_eqdsk
[ -x "$BIN" ] || { echo "make_cfg5_eqdsk: $BIN missing -- run oracle/build_ref.sh where /root/reference is mounted"; exit 1; }
[ $# -gt 0 ] || set -- solovev_2_eqdsk_129.in solovev_2_eqdsk_49x65.in
TOP=$(mktemp -d); trap 'rm -rf "$TOP"' EXIT
for NML in "$@"; do
  OUT=$(sed -n "s/^ *eqdsk_file_name *= *'\([^']*\)'.*/\1/p" "$ROOT/configs/$NML")
  [ -n "$OUT" ] || { echo "make_cfg5_eqdsk: configs/$NML names no eqdsk_file_name"; exit 1; }
  W=$TOP/${NML%.in}; mkdir "$W"
  cp "$ROOT/configs/$NML" "$W/rays.in"
  ( cd "$W" && "$BIN" > solovev_2_eqdsk.log 2>&1 )
  cat "$W/$OUT" > "$ROOT/configs/$OUT"
  echo "configs/$OUT: $(head -c 60 "$ROOT/configs/$OUT" | head -1)"
done
