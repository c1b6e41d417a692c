#!/usr/bin/env python3
"""Register / scratch / LDS figures of every kernel in libhilo_hip.so (or the library given), from the code objects' metadata;
a .hsaco of the run-time compiler's cache is read as the one code object it is.
    python tools/kernel_resources.py [lib.so | file.hsaco] [substring ...]
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
given = len(sys.argv) > 1 and sys.argv[1].endswith(('.so', '.hsaco'))
lib = sys.argv[1] if given else os.path.join(HERE, '..', 'hilo_mpc_amd', 'libhilo_hip.so')
keys = sys.argv[2:] if given else sys.argv[1:]
BIN = '/opt/rocm/lib/llvm/bin'


def code_objects(path, td):
    if path.endswith('.hsaco'):
        yield path
        return
    data = open(path, 'rb').read()
    # the bundles: concatenated "__CLANG_OFFLOAD_BUNDLE__" blobs inside .hip_fatbin; unbundle each by offset
    offs = [m.start() for m in re.finditer(b'__CLANG_OFFLOAD_BUNDLE__', data)]
    for n, o in enumerate(offs):
        end = offs[n + 1] if n + 1 < len(offs) else len(data)
        blob = os.path.join(td, f'b{n}.bin')
        open(blob, 'wb').write(data[o:end])
        co = os.path.join(td, f'b{n}.co')
        r = subprocess.run([f'{BIN}/clang-offload-bundler', '--unbundle', '--type=o', f'--input={blob}', f'--output={co}',
                            '--targets=hipv4-amdgcn-amd-amdhsa--gfx950'], capture_output=True, text=True)
        if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co) > 0:
            yield co


with tempfile.TemporaryDirectory() as td:
    rows = []
    for co in code_objects(lib, td):
        notes = subprocess.run([f'{BIN}/llvm-readelf', '--notes', co], capture_output=True, text=True).stdout
        for blk in notes.split('  - .agpr_count:')[1:]:
            get = lambda k: (re.search(rf'\.{k}:\s+(\S+)', blk) or [None, '?'])[1]   # noqa: E731
            name = get('name')
            dem = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
            rows.append((dem, get('vgpr_count'), re.match(r'\s*(\d+)', blk).group(1), get('private_segment_fixed_size'), get('group_segment_fixed_size')))
    for dem, v, a, sc, lds in sorted(rows):
        if not keys or any(k in dem for k in keys):
            print(f"vgpr {v:>4s} agpr {a:>4s} scratch {sc:>6s} B  lds {lds:>7s} B  {dem[:150]}")
