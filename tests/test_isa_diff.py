"""scripts/isa_diff.py on two tiny hand-written assembly files: a kernel that only moved (other
block-label numbers) is identical, one with another instruction differs (with its counts and
sizes), one present on one side only is reported as such."""
import importlib.util
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "scripts", "isa_diff.py")


def _kernel(sym, fn, body, vgpr=8, lds=0):
    return f"""\t.text
\t.globl\t{sym}
\t.type\t{sym},@function
{sym}:
; %bb.0:
{body}\ts_endpgm
.Lfunc_end{fn}:
\t.size\t{sym}, .Lfunc_end{fn}-{sym}
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {sym}
\t\t.amdhsa_group_segment_fixed_size {lds}
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 16
\t.end_amdhsa_kernel
"""


def _loop(fn, extra=""):
    return (f"\ts_load_dword s0, s[4:5], 0x0\n\tv_mov_b32_e32 v1, 0\n.LBB{fn}_1: ; a comment\n"
            f"\tv_add_u32_e32 v1, 1, v1\n{extra}\tds_write_b32 v0, v1\n\ts_cbranch_scc1 .LBB{fn}_1\n"
            f"\tglobal_store_dword v0, v1, s[2:3]\n")


OLD = _kernel("k_same", 0, _loop(0)) + _kernel("k_changed", 1, _loop(1)) + _kernel("k_gone", 2, _loop(2))
# k_same moved behind k_changed: its function and label numbers change, nothing else
NEW = _kernel("k_changed", 0, _loop(0, "\tv_mul_u32_u24_e32 v1, 3, v1\n"), vgpr=9, lds=64) + _kernel("k_same", 1, _loop(1))


def _module():
    spec = importlib.util.spec_from_file_location("isa_diff", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_relabelled_identical_differing_and_missing_kernels():
    rows = {sym: (verdict, oc, nc) for sym, verdict, oc, nc in _module().diff(OLD, NEW)}
    assert set(rows) == {"k_same", "k_changed", "k_gone"}
    assert rows["k_same"] == ("identical", None, None)
    assert rows["k_gone"] == ("only in OLD", None, None)
    verdict, oc, nc = rows["k_changed"]
    assert verdict == "differs"
    assert oc == {"total": 7, "valu": 2, "salu": 3, "vmem": 1, "lds": 1, "vgpr": 8, "sgpr": 16, "scratch": 0, "lds_bytes": 0}
    assert nc == {"total": 8, "valu": 3, "salu": 3, "vmem": 1, "lds": 1, "vgpr": 9, "sgpr": 16, "scratch": 0, "lds_bytes": 64}
    # the other direction: the kernel is new
    back = {sym: verdict for sym, verdict, _, _ in _module().diff(NEW, OLD)}
    assert back["k_gone"] == "only in NEW" and back["k_same"] == "identical"


def test_command_line_report_and_exit_status(tmp_path):
    old, new = tmp_path / "old.s", tmp_path / "new.s"
    old.write_text(OLD)
    new.write_text(NEW)
    r = subprocess.run([sys.executable, SCRIPT, str(old), str(new)], capture_output=True, text=True)
    assert r.returncode == 1
    assert "identical    k_same" in r.stdout and "differs      k_changed" in r.stdout
    assert "only in OLD  k_gone" in r.stdout
    assert "3 kernels: 1 identical, 1 differs, 1 only in OLD, 0 only in NEW" in r.stdout
    same = subprocess.run([sys.executable, SCRIPT, str(old), str(old), "--kernel", "k_same"],
                          capture_output=True, text=True)
    assert same.returncode == 0 and "1 kernels: 1 identical" in same.stdout
