#!/bin/bash
# Host sanitizer runs of the native core (CPU paths: engines, thread/TCP transports, planner, I/O,
# watchdog).  GPU sanitizers are not used on this pool; the HIP sources are compiled without them.
#   bash tools/sanitize_check.sh [address|thread ...]
set -e
cd "$(dirname "$0")/.."
for san in "${@:-address thread}"; do
  for s in $san; do
    b=${GOL_SAN_BUILD_DIR:-/tmp}/gol-san-$s
    cmake -S . -B $b -DGOL_SANITIZE=$s -DGOL_WITH_PYTHON=OFF -DGOL_WITH_MPI=OFF -DCMAKE_BUILD_TYPE=RelWithDebInfo > $b.log 2>&1
    cmake --build $b -j8 --target gol_unit gol_rule_unit gol_rle_unit gol_bounded_unit gol_census_unit gol_signature_unit gol_nbhd_unit gol_film_unit gol_density_film_unit gol >> $b.log 2>&1
    echo "== $s"
    if [ $s = thread ]; then export OMP_NUM_THREADS=1 TSAN_OPTIONS="halt_on_error=1"; else export ASAN_OPTIONS="detect_leaks=1"; fi
    GOL_BACKEND=cpu $b/gol_unit | tail -1
    $b/gol_rule_unit | tail -1  # rule strings, cpu::superstep under life-like rules
    $b/gol_rle_unit | tail -1   # RLE reader and writer: round trips, every rejection
    $b/gol_bounded_unit | tail -1  # bounded boards: cpu::superstep with dead edges, the RLE topology suffix
    $b/gol_census_unit | tail -1   # census: cpu::superstep's per-generation counts of a tile's own cells
    $b/gol_signature_unit | tail -1  # signatures: cpu::superstep's per-generation hashes, cpu::signature
    $b/gol_nbhd_unit | tail -1  # von Neumann and hexagonal neighbourhoods: rule strings, cpu::superstep under V and H rules
    $b/gol_film_unit | tail -1  # film mode: cpu::superstep's per-generation packed frames of a board window
    $b/gol_density_film_unit | tail -1  # density-film mode: CPU engines' per-generation density maps on 1 to 4 thread ranks
    # the CLI's multi-rank I/O: 2-D dumps routed point to point, a checkpoint written by a 2x2 grid
    # and resumed by 3 strips (thread ranks)
    w=$(mktemp -d)
    (cd $w && GOL_BACKEND=cpu GOL_NRANKS=4 GOL_GLOBAL=1 GOL_DECOMP=2d GOL_GRID=2x2 GOL_CHECKPOINT_EVERY=8 \
        GOL_CHECKPOINT_PATH=$w/ck $b/gol 5 256 16 256 1 > /dev/null &&
     GOL_BACKEND=cpu GOL_NRANKS=3 GOL_GLOBAL=1 GOL_RESTART=$w/ck $b/gol 5 256 24 256 1 > /dev/null &&
     echo "CLI dump/checkpoint run clean" &&
     GOL_BACKEND=cpu GOL_NRANKS=4 GOL_GLOBAL=1 GOL_DECOMP=2d GOL_GRID=2x2 GOL_BOUNDARY=dead GOL_RULE=B36/S23 \
        $b/gol 5 256 16 256 1 > /dev/null && echo "CLI bounded run clean")
    rm -rf $w
  done
done
