"""The one-shot arena's layout without a device: tests/arena_layout_check.cpp runs capi_internal.h's arena_layout / arena_point over lists of
slots whose offsets follow from the rule (256-byte pieces, an empty array takes one byte) and are written out in the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_arena_layout_follows_the_rule(tmp_path):
    exe = str(tmp_path / "arena_layout_check")
    # host code only, with AddressSanitizer and UBSan on the host compilation alone (the headers of the kernel units need hipcc; nothing
    # is compiled for a device); the program links no unit of the library
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-g", "-Wall", *"-Xarch_host -fsanitize=address,undefined".split(), "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "arena_layout_check.cpp")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("DD_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("arena_layout_check: ") and r.stdout.endswith(" checks ok\n"), \
        (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
