"""What a neural network inside a model costs the run-time compiler, without a GPU (HILO_JIT_COMPILE_ONLY=1, private cache):
for the reference test's bioreactor with (mu, Rs, Rfp) learned by networks of growing size, with and without the symbolic
derivative source, the statements of the emitted model, the compile time of the NMPC unit and of the filter / roll-out / LQR unit,
and registers / scratch of every kernel in them.  The thresholds `Model.ANN_SYM_NODES` / `ANN_MAX_NODES` and the table of
DESIGN.md 5.3b come from this script.

    python tools/ann_codesize.py [--only NAME]
"""
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READELF = '/opt/rocm/lib/llvm/bin/llvm-readelf'

NETS = [('2-10-3 sigmoid', (10,), ('sigmoid',)), ('2x8 tanh', (8, 8), ('tanh', 'tanh')), ('2x16 tanh', (16, 16), ('tanh', 'tanh')),
        ('3x16 tanh', (16, 16, 16), ('tanh',) * 3)]


def kernels(cache, before):
    out = []
    for f in sorted(set(os.listdir(cache)) - before):
        if not f.endswith('.hsaco'):
            continue
        notes = subprocess.run([READELF, '--notes', os.path.join(cache, f)], capture_output=True, text=True).stdout
        for blk in notes.split('- .agpr_count')[1:]:
            def get(key):
                m = re.search(rf'\.{key}:\s*(\S+)', blk)
                return m.group(1) if m else '?'
            out.append((get('name'), get('vgpr_count'), get('private_segment_fixed_size'), get('vgpr_spill_count')))
    return out


def main(argv):
    only = argv[argv.index('--only') + 1] if '--only' in argv else None
    cache = tempfile.mkdtemp(prefix='hilo_ann_jit_')
    os.environ['HILO_JIT_CACHE'] = cache
    os.environ['HILO_JIT_COMPILE_ONLY'] = '1'
    from hilo_mpc_amd import EKF, Model
    from tests import ann_reference as ar
    from tests.problems import C2, product_nmpc
    spec = dict(C2, N=5, p=list(ar.P_REST))
    for name, widths, acts in NETS:
        if only and only != name:
            continue
        W, b, acts, xs, ys = ar.bio_net(widths, acts)
        ann = ar.make_ann(ar.FEATURES, ar.LABELS, widths, acts, W, b, xs, ys)
        for symbolic in (True, False):
            Model.ANN_SYM_NODES = 10 ** 6 if symbolic else 0
            Model.ANN_MAX_NODES = 10 ** 6
            m = ar.bioreactor()
            m.substitute_from(ann)
            t0 = time.time()
            src = m.copy().discretize('erk', order=4).setup(dt=1.).user_source()
            t_src = time.time() - t0
            stm = sum(1 for ln in src.splitlines() if ln.strip().startswith('const '))
            print(f"== {name} ({ann.n_nodes()} neurons), symbolic source {'on' if symbolic else 'off'}: {stm} statements, "
                  f"{len(src) // 1024} KiB of source, emitted in {t_src:.1f} s", flush=True)
            for unit, build in (('NMPC N=5', lambda: product_nmpc(spec, model=m.copy())),
                                ('filter / roll-out / LQR', lambda: EKF(m.copy().discretize('erk', order=4).setup(dt=1.)).setup())):
                before = set(os.listdir(cache))
                t0 = time.time()
                try:
                    build()
                except Exception as e:
                    print(f"   {unit}: {type(e).__name__}: {str(e)[:300]}")
                dt = time.time() - t0
                ks = kernels(cache, before)
                worst = max([int(k[2]) for k in ks if k[2].isdigit()] or [0])
                print(f"   {unit}: compiled in {dt:.1f} s, {len(ks)} kernels, largest scratch {worst} B/lane", flush=True)
                for k in ks:
                    print(f"      {k[0][:60]:60s} vgpr {k[1]:>4s} scratch {k[2]:>6s} B spill {k[3]}")


if __name__ == '__main__':
    main(sys.argv[1:])
