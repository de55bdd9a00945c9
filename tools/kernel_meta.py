#!/usr/bin/env python3
"""Resource numbers of every kernel in a built library, from the code objects' metadata (no GPU needed):

  python tools/kernel_meta.py rlcard_amd/libcardsim.so > new.txt
One line per kernel, sorted: mangled name, VGPRs, SGPRs, LDS bytes, scratch bytes, VGPRs spilled, SGPRs spilled. The
library's .hip_fatbin section holds one offload bundle per translation unit; each is unbundled for gfx950 and its notes
read with llvm-readelf. To show that a change to shared code (cs_skeleton.h, cs_device.h) left the existing kernels
alone, build the parent commit in a second worktree, list both libraries and compare the lists without the new game's
lines (`grep -v 5ScoutE new.txt | diff - parent.txt`)."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--' + os.environ.get('ARCH', 'gfx950')
FIELDS = ('name', 'vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size',
          'vgpr_spill_count', 'sgpr_spill_count')


def kernels(lib):
    rows = []
    with tempfile.TemporaryDirectory() as t:
        fat = os.path.join(t, 'fat.bin')
        subprocess.check_call(['objcopy', '-O', 'binary', '--only-section=.hip_fatbin', lib, fat])
        data = open(fat, 'rb').read()
        offs = [m.start() for m in re.finditer(b'__CLANG_OFFLOAD_BUNDLE__', data)] + [len(data)]
        for i in range(len(offs) - 1):
            piece, co = os.path.join(t, 'b%d.bin' % i), os.path.join(t, 'c%d.co' % i)
            with open(piece, 'wb') as f:
                f.write(data[offs[i]:offs[i + 1]])
            subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o',
                                   '--targets=' + TARGET, '--input=' + piece, '--output=' + co])
            if os.path.getsize(co) == 0:
                continue
            notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co]).decode()
            for blk in re.split(r'\n\s*- \.agpr_count', notes)[1:]:
                rows.append(' '.join(re.search(r'\.%s:\s*(\S+)' % k, blk).group(1) for k in FIELDS))
    return sorted(rows)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    print('\n'.join(kernels(sys.argv[1])))
