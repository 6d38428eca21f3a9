#!/bin/bash
# register / scratch / occupancy of the trace_stack_kernel instantiations (compiler view), one line each, built with the Makefile's FLAGS
#   tools/kres.sh [NAME] [-D...]   NAME: print only the instantiations whose name (mangled, or as printed) contains it; -D...: extra flags
#   tools/kres.sh _ZN3svo18trace_stack_kernelILi256ELi12ELi3ELb0ELb0ELb0ELb0E   -> the default instantiation
# template arguments as printed: NS, K, GE, DBG, CNT, SHD (BLOCK 256)
csrc=$(cd "$(dirname "$0")/../octree-tracer_amd/csrc" && pwd)
filt=trace_stack_kernel
if [ $# -gt 0 ] && [ "${1#-}" = "$1" ]; then filt=$1; shift; fi
flags=$(make -s --no-print-directory -C "$csrc" --eval='_flags: ; @echo $(FLAGS)' _flags | sed 's/ -fPIC\b//; s/ -Wall\b//')
cd "$csrc" && ${HIPCC:-/opt/rocm/bin/hipcc} $flags "$@" -c --cuda-device-only -Rpass-analysis=kernel-resource-usage svo_kernels.hip -o /dev/null 2>&1 |
FILT="$filt" python3 -c "
import os, re, sys
filt, cur = os.environ['FILT'], None
for l in sys.stdin:
    m = re.search(r'Function Name: (\S+)', l)
    if m: cur = {'name': m.group(1)}; continue
    if cur is None: continue
    for k, pat in (('vgpr', r' VGPRs: (\d+)'), ('sgpr', r'TotalSGPRs: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('occ', r'Occupancy \[waves/SIMD\]: (\d+)')):
        m = re.search(pat, l)
        if m: cur[k] = m.group(1)
    if 'LDS Size' in l:
        n = cur['name']
        if 'trace_stack_kernel' in n:
            p = re.sub(r'_ZN3svo18trace_stack_kernelILi256E', 'stack<', n); p = re.sub(r'EEEvNS.*', '>', p).replace('ELi', ',').replace('ELb', ',').replace('Li', '')
            if filt in n or filt in p:
                print(p, 'vgpr', cur.get('vgpr'), 'sgpr', cur.get('sgpr'), 'scratch', cur.get('scratch'), 'occ', cur.get('occ'))
        cur = None
"
