#!/usr/bin/env python3
"""Register table of two builds from the compiler's resource remarks.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Rpass-analysis=kernel-resource-usage -c gemm.hip 2> parent_gemm.txt   (each tree)
    python tools/resource_table.py parent_gemm.txt branch_gemm.txt [substring of the demangled name ...]

One line per kernel whose demangled name holds one of the substrings (all kernels without any): VGPRs, AGPRs, scratch bytes per
lane and occupancy in waves per SIMD, first file against second, and a last line that says whether scratch stayed 0 and no occupancy fell.  A kernel of the
second build is named as it is there; where the first build has none of that name it is compared with the first build's kernel of
the name less one trailing integer template argument (`-` if there is none either).
"""
import re
import subprocess
import sys


def parse(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r'remark:.*?\b(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            name = m.group(2)
            out[name] = {}
        else:
            out[name][m.group(1).split(' ')[0]] = int(m.group(2))
    return out


def demangled(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return {re.sub(r'\(.*$', '', re.sub(r'^void algp::', '', d)): n for n, d in zip(names, out)}


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    keys = sys.argv[3:]
    da, db = demangled(list(a)), demangled(list(b))
    ok = True
    print('| kernel | VGPRs | AGPRs | scratch B/lane | occupancy |')
    print('|---|---|---|---|---|')
    def earlier(d):
        """the first build's kernel of this name, or of the name less one trailing integer template argument (a kernel that the
        second build compiles once per value of a new last parameter: GenGemmArgs<T, 2, FAM>, kmat_kernel<T, DP, EQ, FAM>)"""
        if d in da:
            return d
        for m in re.finditer(r', -?\d+>', d):
            cut = d[:m.start()] + '>' + d[m.end():]
            if cut in da:
                return cut
        return None

    for d in list(db) + [d for d in da if d not in db and not any(earlier(e) == d for e in db)]:
        if keys and not any(k in d for k in keys):
            continue
        p, q = a.get(da.get(earlier(d) if d in db else d)), b.get(db.get(d))
        if p and q:
            ok = ok and q['ScratchSize'] == 0 and q['Occupancy'] >= p['Occupancy']
        elif q:
            ok = ok and q['ScratchSize'] == 0
        cells = ['%s -> %s' % (p[k] if p else '-', q[k] if q else '-') for k in ('VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy')]
        print('| `%s` | %s |' % (d, ' | '.join(cells)))
    print('\nscratch 0 and occupancy not below the first build for every kernel listed (a kernel of one build only: scratch 0): %s'
          % ('yes' if ok else 'NO'))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
