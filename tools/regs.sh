#!/bin/bash
# Register / scratch / occupancy / spill / static-LDS report of the env kernels (cross-compiled for gfx950, no GPU;
# the planner kernels' LDS is dynamic -- plan_lds / plan_value_lds in heist_env.hip -- so their LDS Size prints 0).
# usage: tools/regs.sh [regex]   (default: step|reset|cones; `plan` the planner's and the planner
#        field's instances, `field` plan_field_kernel's alone, `value` plan_value_kernel's alone,
#        `masked` plan_masked_kernel's alone, `place` plan_place_kernel's and plan_place_guard_kernel's,
#        `walls` plan_walls_kernel's alone)
#        tools/regs.sh play      plan_play_kernel (heist_play.hip), with its SGPRs and LDS
#        tools/regs.sh q         plan_q_kernel (heist_q.hip), the same columns
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=$ROOT/rl-project-heist-architect-adversarial-reinforcement-learning-framework-cse4019_amd/csrc
OUT=$(mktemp -d)
if [ "$1" = "play" ] || [ "$1" = "q" ]; then
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math --offload-arch=gfx950 \
    -I "$ROOT/include" -I "$CSRC" -c "$CSRC/heist_$1.hip" -o "$OUT/hp.o" -Rpass-analysis=kernel-resource-usage \
    > "$OUT/res.txt" 2>&1 || { grep -E "error" "$OUT/res.txt" | head -20; exit 1; }
  grep -E "remark: +(Function Name|TotalSGPRs:|VGPRs:|Occupancy|SGPRs Spill|VGPRs Spill|ScratchSize|LDS Size)" "$OUT/res.txt" \
    | sed 's/.*remark: *//; s/ \[-Rpass.*//' | paste - - - - - - - - | sed 's/Function Name: _ZN5heist[0-9_A-Za-z]*N_1[0-9]*//; s/ENS_[^\t]*//'
  rm -rf "$OUT"
  exit 0
fi
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math ${HEIST_ENV_FLAGS:--fno-slp-vectorize -mllvm -disable-machine-licm} --offload-arch=gfx950 \
  -I "$ROOT/include" -I "$CSRC" -c "$CSRC/heist_env.hip" -o "$OUT/he.o" -Rpass-analysis=kernel-resource-usage \
  > "$OUT/res.txt" 2>&1 || { grep -E "error" "$OUT/res.txt" | head -20; exit 1; }
grep -E "remark: +(Function Name|VGPRs:|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)" "$OUT/res.txt" | sed 's/.*remark: *//; s/ \[-Rpass.*//' \
  | paste - - - - - - - | sed 's/Function Name: _ZN5heist//; s/EEEvNS[^\t]*//' | grep -E "${1:-step|reset|cones}"
rm -rf "$OUT"
