#!/bin/bash
# Forward vs adjoint ms per time step at C2 and C3 (2 channels x 2 times), then one kernel-trace profile of a C3 adjoint
# call (rocprofv3 --kernel-trace --stats; k_adj_strengths / k_adj_accumulate appear in its kernel statistics).
# Then the lattice path (--lattice: the reference's default call, the type-1 forward) at C2, C3 and C3 with 32 channels,
# with the type-3 and the type-2 adjoint, and a kernel-trace profile of one type-2 C3 call.  PARENT=<checkout of an
# earlier commit, built in place> adds the same lattice calls against that checkout's package (its adjoint there is the
# type-3 transform): the yardstick the type-2 adjoint is measured against.
# Every GPU step has its own time limit, and the script stops at the first step that fails (its exit status is the
# step's: 124 / 137 a time limit, 134 an abort, 139 a segmentation fault).
# Usage: tools/adjoint_timing.sh [output directory, default profiles/adjoint]
set -uo pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/adjoint}
mkdir -p "$OUT"
step() {  # output file, seconds, command...
    local out=$1 secs=$2
    shift 2
    timeout -k 10 "$secs" "$@" > "$out"
    local rc=$?
    cat "$out"
    if [ $rc -ne 0 ]; then
        echo "adjoint_timing: '$*' failed with status $rc; nothing more is started" >&2
        exit $rc
    fi
}
step "$OUT/timing_c2.json" 300 python tools/pass_timing.py --family adjoint --config C2
step "$OUT/timing_c3.json" 600 python tools/pass_timing.py --family adjoint --config C3
step "$OUT/rocprof.log" 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o adj_c3 -- \
    python tools/pass_timing.py --family adjoint --config C3 --profile adjoint
find "$OUT/trace" -name "*kernel_stats.csv" -exec cp {} "$OUT/c3_adjoint_kernel_stats.csv" \;
for c in "C2 2" "C3 2" "C3 32"; do
    set -- $c
    tag=$(echo "$1" | tr A-Z a-z)_${2}ch
    if [ -n "${PARENT:-}" ]; then
        step "$OUT/lattice_parent_${tag}.json" 600 python tools/pass_timing.py --family adjoint --config "$1" --nfreq "$2" --lattice --package "$PARENT"
    fi
    step "$OUT/lattice_type3_${tag}.json" 600 python tools/pass_timing.py --family adjoint --config "$1" --nfreq "$2" --lattice --adjoint-path type3
    step "$OUT/lattice_type2_${tag}.json" 600 python tools/pass_timing.py --family adjoint --config "$1" --nfreq "$2" --lattice --adjoint-path type2
done
step "$OUT/rocprof_type2.log" 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_type2" -o adj2_c3 -- \
    python tools/pass_timing.py --family adjoint --config C3 --lattice --adjoint-path type2 --profile adjoint
find "$OUT/trace_type2" -name "*kernel_stats.csv" -exec cp {} "$OUT/c3_type2_adjoint_kernel_stats.csv" \;
