"""Run one of the tests/cpp host programs (quadrupedal_loco_amd.build.HOST_EXES)
from a GPU test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(name, args=(), input=None, timeout=120):
    """tests/cpp/_build/<name> with `args` and `input` on stdin, built first
    when it is missing.  Asserts exit code 0 and "ALL OK" on stdout; returns
    the completed process (text mode)."""
    exe = os.path.join(ROOT, "tests", "cpp", "_build", name)
    if not os.path.exists(exe):
        from quadrupedal_loco_amd import build
        assert build.build_host_exe(name) == exe
    r = subprocess.run([exe] + [str(a) for a in args], input=input, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r
