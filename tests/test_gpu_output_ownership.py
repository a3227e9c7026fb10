"""The likelihood kernels write every element they own and nothing else: poisoned, guarded result buffers on both entries, both models.

The parity tests compare values, into buffers that already held them: the device-pointer path starts from torch.zeros, where 0 is the most
common expected value, and the host-pointer path reuses one arena per thread, where the second build run on a batch finds the first one's
results at the addresses it is about to write.  Here every result buffer starts out as bytes 0x5A inside 256-byte guards of 0xA5
(tests/_output_ownership.py), the arena's output region included (DD_POISON_OUTPUTS), and after each call every element of
must_write()'s mask is bit-equal to the oracle and every other byte still holds its sentinel.

The contract, per pair status (tests/_output_ownership.must_write; read from the header and the kernels' stores, not from a run):
  DD_PAIR_OK           everything                                      include/dindel_hmm.h:165-185, hmm_kernel.hip:1269-1447,
                                                                       faster_kernel.hip:136-161, :301-310, faster_pair_end.inc
  DD_PAIR_NAN, _LLPOS  main model: everything (the status comes last)  hmm_kernel.hip:1400-1402
  DD_PAIR_NAN          --faster: status, ll = 0, offHapHMQ = 1, zeros in offHap and the nine defaulted values, coverage flags 0;
                       no firstBase / lastBase / hpos                   faster_kernel.hip:136-161
  DD_PAIR_HAPSIZE      main: status, ll = 0, both coverage flags 0      hmm_kernel.hip:576-589 (mark_hapsize)
                       --faster: as its DD_PAIR_NAN                     faster_kernel.hip:136-161
  DD_PAIR_UNSUPPORTED  status, ll = 0, offHap = offHapHMQ = 1           include/dindel_hmm.h:68-71, hmm_kernel.hip:183-189,
                                                                       faster_kernel.hip:73-82
  onHap                every read of the launch, windows without haplotypes included       hmm_kernel.hip:1459-1481, host_path.cpp:148

Left out of the mask, measured on the oracle (tests/test_output_ownership_cpu.py prints and bounds them): at most 22 of 950 pairs and 13 of
350 (3.7 %) are not DD_PAIR_OK in a scenario batch, at most 186 of 45,202 hpos elements (0.4 %) are unwritten; the hand-built edges batch
has 36 pairs, 4 of them DD_PAIR_HAPSIZE and, under --faster, one DD_PAIR_NAN, and 120 (121) of its 1,191 hpos elements are unwritten.

Legs per batch and model, all against one oracle run:
  device    GuardedDevice around DeviceBatch.launch() / launch_faster(); a second launch leaves the buffers byte-identical; a run over
            bodies of 0x00 gives the same owned elements
  host      pageable arrays full of poison and DD_POISON_OUTPUTS=1, under each launch mode of tests/test_gpu_persistent_rounds.MODES
            (--faster: each DD_FAST_GROUPS setting): a value that is not copied back shows as well
  pinned    page-locked arrays written in place, inside guards
  null      (30-bp batch) result pointers the header allows to be NULL"""
import ctypes as C
import os
import time

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import result_lengths
from tests import _output_ownership as oo
from tests import _path_scenarios as ps
from tests.test_gpu_persistent_rounds import KEYS, MODES

pytestmark = pytest.mark.gpu

NAMES = list(oo.batches())
CASES = [pytest.param(name, faster, id="%s-%s" % (name, "faster" if faster else "main")) for name in NAMES for faster in (False, True)]
ENV_KEYS = KEYS + ("DD_FAST_GROUPS",)
OPTIONAL = [k for k, _t in capi.RESULT_FIELDS if k not in ("ll", "status")]


@pytest.fixture(scope="module")
def lib():
    return capi.load()


@pytest.fixture()
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    yield
    for k in ENV_KEYS:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


def set_env(env):
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)


def host_call(lib, p, pb, res, faster):
    """One host-pointer call over a poisoned arena -> the main model's launch records."""
    b = pb.ctypes_batch()
    call = lib.dd_compute_likelihoods_faster if faster else lib.dd_compute_likelihoods
    with oo.poisoned_arena():
        rc = call(C.byref(p), C.byref(b), C.byref(res), 0)
    assert rc == 0, capi.last_error()
    return [] if faster else capi.launch_log()


def last_groups(lib):
    ll = np.zeros(8, np.int32)
    lib.dd_last_launch(C.byref((C.c_int32 * 8).from_buffer(ll)))
    return int(ll[0])


def raw_bytes(g):
    import torch
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().copy() for k, t in g.raw.items()}


def launch(dev, faster):
    import torch
    (dev.launch_faster if faster else dev.launch)()
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,faster", CASES)
def test_every_owned_element_is_written_and_nothing_else(lib, clean_env, name, faster):
    from dindel_tgi_amd.device import DeviceBatch
    t0 = time.time()
    pb, _index, p, want, own = oo.case(name, faster)
    n = result_lengths(pb)
    tag = "%s, %s" % (name, "--faster model" if faster else "main model")

    # device: torch's buffers replaced by poisoned, guarded ones
    dev = DeviceBatch(pb, p, "cuda:0")
    g = oo.GuardedDevice(dev)
    launch(dev, faster)
    kernels = {ps.kernel_name(r) for r in ([] if faster else capi.launch_log())}
    first = dev.results()
    oo.assert_owned(first, want, pb, own, tag + ", device-pointer path")
    g.check(tag + ", device-pointer path")
    before = raw_bytes(g)
    launch(dev, faster)                                                            # the same buffers, not poisoned again
    after = raw_bytes(g)
    for k in before:
        assert np.array_equal(before[k], after[k]), "%s, second launch into the same buffers: %s changed at byte %d" % (
            tag, k, int(np.nonzero(before[k] != after[k])[0][0]) - oo.GUARD)
    g.fill(0x00)                                                                   # what the buffers held does not reach the results
    launch(dev, faster)
    zero = dev.results()
    g.check(tag + ", device-pointer path over zeros")
    for k, _t in capi.RESULT_FIELDS:
        a, b = first[k][:n[k]][own.write[k]], zero[k][:n[k]][own.write[k]]
        assert a.tobytes() == b.tobytes(), "%s: %s depends on what the buffer held (owned element %d)" % (tag, k, int(np.nonzero(a != b)[0][0]))
        assert not zero[k][:n[k]][~own.write[k]].any(), "%s: %s: an element the library does not own was written over zeros" % (tag, k)
    del g, dev

    # host, pageable: poison in the caller's arrays and in the arena, every launch mode
    groups = set()
    for env in ([{}, {"DD_FAST_GROUPS": "2"}, {"DD_FAST_GROUPS": "1"}] if faster else MODES):
        set_env(env)
        arrs, res = oo.alloc_poisoned(pb)
        log = host_call(lib, p, pb, res, faster)
        assert lib.dd_last_direct_outputs() == 0
        kernels |= {ps.kernel_name(r) for r in log}
        if faster:
            groups.add(last_groups(lib))
        oo.assert_owned(arrs, want, pb, own, "%s, host path, pageable, environment %r%s" % (tag, env, "".join("; " + ps.kernel_name(r) for r in log)))
    set_env({})
    # the switch itself: into zeroed arrays, what the library does not own comes back as the arena's poison
    from dindel_tgi_amd.batch import alloc_result
    arrs, res = alloc_result(pb, fill=None)
    host_call(lib, p, pb, res, faster)
    assert (~own.write["hpos"]).any()
    for k, _t in capi.RESULT_FIELDS:
        left = np.ascontiguousarray(arrs[k][:n[k]][~own.write[k]]).view(np.uint8)
        assert (left == oo.BODY_BYTE).all(), "%s: DD_POISON_OUTPUTS did not reach %s" % (tag, k)
    if faster:
        assert groups == {4, 2, 1}, groups
    else:
        assert len(kernels) >= 2, kernels

    # host, page-locked: written in place, inside guards (status and offHapHMQ come through the arena)
    pinned = oo.Guarded(lib, pb)
    try:
        host_call(lib, p, pb, pinned.res, faster)
        assert lib.dd_last_direct_outputs() > 0, lib.dd_last_direct_outputs()
        oo.assert_owned(pinned.arrays(), want, pb, own, tag + ", host path, page-locked")
        pinned.check_guards(tag + ", host path, page-locked")
    finally:
        pinned.release()
    print("ownership %s: %.1f s; %d kernels" % (tag, time.time() - t0, len(kernels)))


def host_run(lib, p, pb, faster, null=()):
    arrs, res = oo.alloc_poisoned(pb)
    for k in null:
        setattr(res, k, None)
    host_call(lib, p, pb, res, faster)
    return arrs


def device_run(p, pb, faster, null=()):
    from dindel_tgi_amd.device import DeviceBatch
    dev = DeviceBatch(pb, p, "cuda:0")
    g = oo.GuardedDevice(dev)
    for k in null:
        setattr(dev.dr, k, None)
    launch(dev, faster)
    g.check("device-pointer path, NULL %r" % (null,))
    return dev.results()


def poison_only(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == oo.BODY_BYTE).all())


@pytest.mark.parametrize("faster", [False, True], ids=["main", "faster"])
@pytest.mark.parametrize("path", ["host", "device"])
def test_null_result_pointers(lib, clean_env, path, faster):
    """include/dindel_hmm.h: any result pointer but ll and status may be NULL, then it is not written.  The arrays that are asked for come
    out byte for byte as in the full run, what a NULL pointer's buffer held stays (nothing is written through a stale address), and onHap:
    the host-pointer entries derive it from a device copy of offHapHMQ of their own (host_path.cpp describe()); the device-pointer entries
    skip the pass when either pointer is NULL (launch.cpp want_onhap)."""
    name = NAMES[0]
    assert name.startswith("hap30-")
    pb, _index, p, want, own = oo.case(name, faster)
    run = (lambda null: host_run(lib, p, pb, faster, null)) if path == "host" else (lambda null: device_run(p, pb, faster, null))
    full = run(())
    oo.assert_owned(full, want, pb, own, "full run, %s path" % path)
    n = result_lengths(pb)

    got = run(tuple(OPTIONAL))
    for k in ("ll", "status"):
        assert got[k][:n[k]].tobytes() == full[k][:n[k]].tobytes(), (path, "every optional pointer NULL", k)
    for k in OPTIONAL:
        assert poison_only(got[k]), (path, "every optional pointer NULL", k)

    for null in ("hpos", "offHapHMQ", "onHap"):
        got = run((null,))
        assert poison_only(got[null]), (path, null)
        for k, _t in capi.RESULT_FIELDS:
            if k == null:
                continue
            if k == "onHap" and null == "offHapHMQ" and path == "device":
                assert poison_only(got[k]), "onHap was written without offHapHMQ on the device-pointer path"
                continue
            assert got[k][:n[k]].tobytes() == full[k][:n[k]].tobytes(), "%s path, %s NULL: %s differs from the full run at element %d" % (
                path, null, k, int(np.nonzero(got[k][:n[k]] != full[k][:n[k]])[0][0]))
