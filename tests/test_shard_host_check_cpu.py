"""The host paths of avatar_amd/csrc/avt_shard.cpp that need no device - the packed model and every refusal that returns before a device is
touched - walked by tests/cpp/shard_host_check.cpp, a program with its own main that links avt_shard.cpp alone and is built with the host's
address and undefined-behaviour sanitizers (no GPU, nothing loaded into Python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avatar_amd", "csrc")


def test_shard_host_paths_under_the_host_sanitizers():
    b = subprocess.run(["make", "-C", CSRC, "shard_host_check_san"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-1500:] + b.stderr[-3000:]
    r = subprocess.run([os.path.join(CSRC, "shard_host_check_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failed" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
