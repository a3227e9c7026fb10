"""The launch geometry without a device: tests/launch_shape_check.cpp (plan.cpp and batch_host.cpp only, no kernel unit) shapes every launch
recorded in tests/golden/launch_shapes.json from its scalars and switches and must reproduce the dd_launch_log records, dd_last_launch and
dd_kernel_name that the real launches left (tests/_launch_shapes.py describes the fixture)."""
import os
import subprocess

from tests import _launch_shapes as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dindel_tgi_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def case_lines(case):
    out = ["case " + case["name"], "params %s %d" % (case["params"], -1 if case["maxLengthDel"] is None else case["maxLengthDel"])]
    out += ["env %s %s" % kv for kv in sorted(case["env"].items())]
    for a in case["asks"]:
        rec = a["record"]
        out.append("ask " + " ".join(str(a[k]) for k in ls.ASK_FIELDS) + (" 1 " + " ".join(map(str, rec)) if rec is not None else " 0"))
    out += ["last " + " ".join(map(str, case["last_launch"])), "name " + case["kernel_name"], "end"]
    return out


def test_shape_functions_reproduce_the_recorded_launches(tmp_path):
    cases = ls.load_cases()
    assert len(cases) >= 40 and len({c["name"] for c in cases}) == len(cases)
    exe, txt = str(tmp_path / "launch_shape_check"), str(tmp_path / "cases.txt")
    # host code only, with AddressSanitizer and UBSan on the host compilation alone (the headers of the kernel units need hipcc; nothing
    # is compiled for a device); the two library units link without any kernel unit
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-g", "-Wall", *"-Xarch_host -fsanitize=address,undefined".split(), "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "launch_shape_check.cpp"), os.path.join(CSRC, "plan.cpp"), os.path.join(CSRC, "batch_host.cpp")])
    with open(txt, "w") as f:
        f.write("\n".join(line for c in cases for line in case_lines(c)) + "\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DD_")}
    r = subprocess.run([exe, txt], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    n_asks = sum(len(c["asks"]) for c in cases)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "launch_shape_check: %d cases, %d asks ok\n" % (len(cases), n_asks), \
        (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
