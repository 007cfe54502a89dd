"""Static checks of the built GEMM code (CPU only; hipcc cross-compiles gfx950 without a GPU)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_pp256_operand_loads_keep_their_registers():
    """The pp256 epilogue loads its fused operands with inline asm and hand-counted waits; a register copy between such a
    load and its wait would read stale data (it happened once: two sibling request sites, NaNs in the gated-residual
    epilogue).  scripts/check_pp_asm.py compiles gemm_pp.hip to assembly and asserts that every request site of a kernel's
    main loop writes the same physical registers and that no kernel spills VGPRs (scratch traffic would also break the
    counted vmcnt waits)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_pp_asm.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("-> ok") >= 3, r.stdout


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_w4_compiler_stays_out_of_the_k_loops_registers():
    """The w4 GEMM's k-loop is generated inline asm on LITERAL registers (a[0:255], v[96:255]); v[144:255] hold data across an
    epilogue.  hipcc once overran a budget of 96 registers instead of spilling (v96 / v97 handed out as temporaries: the first staging
    register corrupted in every tile but a workgroup's first).  scripts/check_w4_asm.py compiles gemm_w4.hip to assembly and asserts
    that no compiler-generated instruction of any w4 kernel names v144+ or an accumulator register, and that nothing is spilled to
    scratch."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_w4_asm.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "10 w4 kernels, 0 problem lines" in r.stdout, r.stdout


def test_committed_w4_k_loop_is_what_the_generator_writes(tmp_path):
    """csrc/gemm_w4_acc.inc is generated (scripts/gen_w4_acc.py): a hand edit, or a generator change not rerun, is caught here."""
    out = tmp_path / "gemm_w4_acc.inc"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_w4_acc.py"), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(ROOT, "micro_diffusion_amd", "csrc", "gemm_w4_acc.inc")) as fh:
        assert out.read_text() == fh.read()


def _reached(path, seen):
    """Every file `path` reaches through #include "..." (and gemm_w4.hip's default W4_ACC_INC), resolved as the builds resolve them:
    the including file's directory, then include/."""
    text = open(path).read()
    for name in re.findall(r'^\s*#\s*(?:include|define\s+W4_ACC_INC)\s+"([^"]+)"', text, re.M):
        found = [f for f in (os.path.join(os.path.dirname(path), name), os.path.join(ROOT, "include", name)) if os.path.isfile(f)]
        assert found, f"{path}: #include \"{name}\" not found"
        f = os.path.realpath(found[0])
        if f not in seen:
            seen.add(f)
            _reached(f, seen)
    return seen


@pytest.mark.parametrize("binding", ["hip", "comm", "mds", "probes"])
def test_library_hash_covers_every_included_file(binding):
    """A library is rebuilt when the hash of its inputs changes: every file its sources include must be among them, or an edit of
    that file leaves the old library loaded."""
    from micro_diffusion_amd import comm, hip, mds
    from tests import probes
    csrc = os.path.join(ROOT, "micro_diffusion_amd", "csrc")
    srcs, hashed = {"hip": ([os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hip")], hip._hashed_files()),
                    "comm": ([comm._SRC], comm._HASHED), "mds": ([mds._SRC], mds._HASHED), "probes": ([probes._SRC], probes._HASHED)}[binding]
    reached = {os.path.realpath(s) for s in srcs}
    for s in srcs:
        _reached(s, reached)
    assert reached - {os.path.realpath(f) for f in hashed} == set()
