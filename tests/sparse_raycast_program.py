"""Builds and runs tools/sparse_raycast_check.cpp -- the host check of csrc/sparse_raycast_grid.h (the render index with its bounded probe, the corner
arithmetic and the flag rule of the ray-caster of the sparse TSDF volume) -- with the host compiler.  The program is a stand-alone
executable: nothing is loaded into the Python process.  tests/test_sparse_raycast_reference.py (CPU) builds it under the address and
undefined-behaviour sanitizers.  Each result is computed once per process."""
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SOURCE = os.path.join(ROOT, "tools", "sparse_raycast_check.cpp")


def host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


@functools.lru_cache(maxsize=None)
def run(sanitize):
    """(status, output): status None when there is no host compiler, else the program's exit status (a failed build counts as 1).
    ``sanitize``: build with ``-fsanitize=address,undefined`` (for tests that run on a CPU machine only)."""
    compiler = host_compiler()
    if compiler is None:
        return None, "no host compiler"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sparse_raycast_check")
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        build = subprocess.run([compiler, "-std=c++17", "-O1", "-g", *flags, SOURCE, "-o", exe], capture_output=True, text=True)
        if build.returncode != 0:
            return 1, build.stdout + build.stderr
        done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        return done.returncode, done.stdout + done.stderr
