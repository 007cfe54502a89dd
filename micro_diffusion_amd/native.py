"""Build and load the project's native libraries: one protocol for every ctypes binding (hip, comm, mds, tests/probes) and one compile
line for the static audits of the kernels.

A library is up to date when `.<libname>.hash` next to it holds the digest of what its build reads (sources, headers, flags).  The
check needs no lock, so a read-only install loads; a stale library is rebuilt under an exclusive lock on `.<libname>.lock` (every
rank of a node may find it stale at once), linked to a name of the building process and renamed into place, so no process can
dlopen a half-written file."""
from __future__ import annotations

import ctypes
import fcntl
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "micro_diffusion_amd", "csrc")


def hipcc() -> str:
    path = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return path if os.path.exists(path) else "hipcc"


def source_hash(files, flags) -> str:
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(flags).encode())
    return h.hexdigest()


def _side_file(lib_path: str, ext: str) -> str:
    d, name = os.path.split(lib_path)
    return os.path.join(d, "." + os.path.splitext(name)[0] + ext)


def up_to_date(lib_path: str, digest: str) -> bool:
    try:
        with open(_side_file(lib_path, ".hash")) as fh:
            return fh.read().strip() == digest and os.path.exists(lib_path)
    except FileNotFoundError:
        return False


def build(lib_path: str, digest: str, make, force: bool = False) -> str:
    """Bring lib_path up to date with digest: make(tmp) writes the library to the file tmp."""
    if not force and up_to_date(lib_path, digest):
        return lib_path
    with open(_side_file(lib_path, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)          # released when the file closes
        if not force and up_to_date(lib_path, digest):
            return lib_path                       # another process built it while this one waited
        tmp = f"{lib_path}.{os.getpid()}.tmp"
        try:
            make(tmp)
            os.replace(tmp, lib_path)
        finally:
            if os.path.exists(tmp):
                os.unlink(tmp)
        with open(_side_file(lib_path, ".hash"), "w") as fh:
            fh.write(digest)
    return lib_path


def run(*cmds, verbose: bool = False) -> None:
    """Run the commands in parallel; raise with the output of the first that fails (verbose: echo what the others print)."""
    procs = [(cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)) for cmd in cmds]
    failed = None
    for cmd, p in procs:
        out = p.communicate()[0].decode(errors="replace")
        if p.returncode != 0 and failed is None:
            failed = f"{os.path.basename(cmd[0])} failed:\n{' '.join(cmd)}\n{out}"
        elif verbose and out.strip():
            sys.stderr.write(out)
    if failed:
        raise RuntimeError(failed)


def load(path: str, sigs, abi_symbol: str | None = None, abi_version: int | None = None) -> ctypes.CDLL:
    """CDLL(path) with restype / argtypes declared from sigs {name: (restype, argtypes)} (a missing symbol raises
    AttributeError: header and library disagree), then the library's ABI version checked against the binding's."""
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if abi_symbol is not None and getattr(lib, abi_symbol)() != abi_version:
        raise RuntimeError(f"{os.path.basename(path)} reports ABI version {getattr(lib, abi_symbol)()}, this binding is written for "
                           f"{abi_version}; rebuild")
    return lib


def compile_csrc(src: str, flags, out: str, *extra: str) -> str:
    """Compile csrc/<src> (or the path src) the way the library build does, plus the extra flags; return the compiler's stderr."""
    r = subprocess.run([hipcc(), *flags, *extra, "-I", INCLUDE, os.path.join(CSRC, src), "-o", str(out)],
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr[-2000:]}")
    return r.stderr


_FIELDS = {"vgprs": r"VGPRs", "spill": r"VGPRs Spill", "scratch": r"ScratchSize \[bytes/lane\]", "lds": r"LDS Size \[bytes/block\]",
           "occ": r"Occupancy \[waves/SIMD\]"}


def resource_usage(src: str, flags, out: str) -> dict:
    """{kernel: {vgprs, spill, scratch, lds, occ}} of the gfx950 code of csrc/<src> (-Rpass-analysis=kernel-resource-usage)."""
    res = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", compile_csrc(src, flags, out, "-c", "-Rpass-analysis=kernel-resource-usage"))[1:]:
        name = b.split()[0]
        res[name] = {}
        for key, label in _FIELDS.items():
            m = re.search(label + r": (\d+)", b)
            assert m, (label, name)
            res[name][key] = int(m.group(1))
    return res
