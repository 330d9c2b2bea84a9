"""bench.py's command line, CPU only: what is refused before any device is touched."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=120, text=True)


def test_conv_layers_needs_full():
    """--conv-layers is written by the per-kernel event pass, which only a --full run makes."""
    r = _bench("--gpus", "1", "--steps", "1", "--warmup", "0", "--conv-layers", os.devnull)
    assert r.returncode == 2 and "--conv-layers" in r.stderr and "--full" in r.stderr, r.stderr[-2000:]
    assert r.stdout == ""


def test_full_is_an_option():
    r = _bench("--help")
    assert r.returncode == 0 and "--full" in r.stdout, r.stdout[-2000:]
