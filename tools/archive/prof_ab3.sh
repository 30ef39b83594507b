#!/bin/bash
# kernel trace of tools/fine_ab.py at 256^3 (library path).  (Its second half traced tools/probe/fine_probe, removed with k_fine_dma; last present at commit 6370176)
export TMPDIR=/tmp
cd /tmp
R=$GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats -d $R/gpurun_out/prof_ab_lib -- python $R/tools/fine_ab.py 256 256 256 > /dev/null 2>&1
python $R/profiles/summarize_rocpd.py $(find $R/gpurun_out/prof_ab_lib -name "*.db" | head -n 1) | head -8 | cut -c1-150
find $R/gpurun_out/prof_ab_lib -name "*.db" -delete
