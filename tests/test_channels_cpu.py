"""The window loop's hand-overs on their own (host/batch_channels.hpp: Channel, OrderedChannel, BatchPool): tests/channels_check.cpp is a
stand-alone program (own main, standard library only, a few threads, small caps) that checks order, blocking at the cap and at the ordered
channel's door, close against abort, and the recycled-batch pool.  Every wait in it has a deadline; the run here has one more."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_channels_check_program(tmp_path):
    exe = str(tmp_path / "channels_check")
    subprocess.check_call(["g++", "-std=c++11", "-pthread", "-O1", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "channels_check.cpp")])
    r = subprocess.run(["timeout", "-k", "5", "60", exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().split("\n")[-1] == "channels_check: ok", (r.returncode, r.stdout, r.stderr)
