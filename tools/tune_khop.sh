#!/bin/bash
# Rebuild graph_sets.hip with different border-BFS settings and time the border stage (tools/khop_probe.py).
#   bash tools/tune_khop.sh "-DK1_TAKE=4" "-DK1_LONG=256" ...     (the tunables: K1_INFLIGHT, K1_LONG, K1_TAKE, KB_TAKE)
for flags in "" "$@"; do
  touch subgnn_amd/csrc/graph_sets.hip
  SGNN_HIPCC_FLAGS="$flags" python -m subgnn_amd.build > /dev/null 2>&1
  echo "[$flags]: $(python tools/khop_probe.py 2>&1 | grep -v amdgpu.ids | grep '43 slots' | head -1)"
done
touch subgnn_amd/csrc/graph_sets.hip
python -m subgnn_amd.build > /dev/null 2>&1
