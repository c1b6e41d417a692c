"""Build guard (tools/check_exec_prologue.py), the head of an else-region: a join block that opens with `s_andn2_saveexec_b64` (or
`s_or_saveexec_b64` / `s_xor_saveexec_b64`) enables the lanes of the saved mask when it is entered with EXEC == 0, so the copies
behind it belong to the else-branch and execute for its lanes; copies in FRONT of it execute for no lane and are reported, and
`s_and_saveexec_b64` enables nothing.  The failure exits of the error-controlled integrator (`return c.status = ...` inside the step
loop of csrc/hilo_integrate.h) compile to such regions in run-time compiled roll-out kernels."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import check_exec_prologue as guard                                                             # noqa: E402


def _listing(body):
    lines = ['0000000000001000 <k>:', '\ts_and_saveexec_b64 s[0:1], vcc // 000000001000: AAAAAAAA',
             '\ts_cbranch_execz 1 // 000000001004: BF880001', '\tv_add_f64 v[0:1], v[0:1], v[2:3] // 000000001008: AAAAAAAA']
    a = 0x100c
    for ins in body:
        lines.append(f'\t{ins} // {a:012X}: AAAAAAAA')
        a += 4
    return '\n'.join(lines) + '\n'


def _hits(body, monkeypatch):
    class R:
        stdout = _listing(body)
    monkeypatch.setattr(subprocess, 'run', lambda cmd, **kw: R())
    return guard.check('x')


def test_copies_of_an_else_branch_are_not_a_prologue(monkeypatch):
    tail = ['v_mov_b32_e32 v0, 1', 'v_mov_b32_e32 v47, v176', 's_or_b64 exec, exec, s[0:1]', 's_endpgm']
    for head in ('s_andn2_saveexec_b64 s[0:1], s[0:1]', 's_or_saveexec_b64 s[2:3], s[2:3]', 's_xor_saveexec_b64 s[2:3], s[2:3]'):
        assert _hits([head] + tail, monkeypatch) == []
        # the same copies in front of it execute for no lane
        assert len(_hits(['v_mov_b32_e32 v47, v176', head] + tail, monkeypatch)) == 1
    # EXEC & mask stays 0: nothing is enabled, the copies behind it are still dead
    assert len(_hits(['s_and_saveexec_b64 s[4:5], s[2:3]'] + tail, monkeypatch)) == 1
    assert len(_hits(tail, monkeypatch)) == 1
