"""Every environment variable the shipped library reads (first table) that no other test sets, one case per
setting: M4RI_HIP_M4RM_CFG (the nine accepted variants and one that is not), M4RI_HIP_APACK, M4RI_HIP_PLAIN_APACK,
M4RI_HIP_SPLITK_WS_MIB, M4RI_HIP_STRASSEN_LEAF_MIN, M4RI_HIP_STRASSEN_MAX_LEVELS, M4RI_HIP_STRASSEN_PAD, M4RI_HIP_HOST_PIPELINE_BLOCKS,
M4RI_HIP_TRANSPOSE_GPU_MIN_BITS, M4RI_HIP_PIN_MIN_BYTES and M4RI_HIP_PIN_CACHE_BYTES.

The library reads most of them once per process, so every case runs in a fresh child process (tests/switch_child.py holds the
bodies), one child at a time.  A child (a) shows that its setting took effect -- the plan queries, read at run time, and the launch
census before and after every product: the forced kernel family ran and no other -- and (b) compares the bits of every product with
the C oracle on full matrices, plain and accumulate form; results that are not views have zero excess bits.  The children inherit
M4RI_HIP_KERNEL_CENSUS_FILE, so their launches count in tests/test_zz_kernel_census.py.

No observable of its effect exists for M4RI_HIP_HOST_PIPELINE_BLOCKS (the block count of the host pipeline is internal), nor for
M4RI_HIP_PIN_MIN_BYTES / M4RI_HIP_PIN_CACHE_BYTES (where a host block lives is internal): those cases compare bits only.

A child that ends by a signal, by an abort, by its time limit, or with a failure whose output names a HIP error is a finding about the library: the remaining
cases of this file are skipped (nothing more is started on the device from here) and say why."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("M4RI_HIP_M4RM_CFG", "M4RI_HIP_APACK", "M4RI_HIP_PLAIN_APACK", "M4RI_HIP_SPLITK_WS_MIB", "M4RI_HIP_STRASSEN_LEAF_MIN",
            "M4RI_HIP_STRASSEN_MAX_LEVELS", "M4RI_HIP_STRASSEN_PAD", "M4RI_HIP_HOST_PIPELINE_BLOCKS", "M4RI_HIP_TRANSPOSE_GPU_MIN_BITS", "M4RI_HIP_PIN_MIN_BYTES",
            "M4RI_HIP_PIN_CACHE_BYTES")

_crashed = None  # why nothing more is started: the first child that ended by a signal, an abort, a device error or its time limit
# a failed child whose output names one of these met an error of the device or the runtime, not a wrong bit: nothing more is started
DEVICE_TROUBLE = re.compile(r"HipError|HIP error|hipError|launch failure|illegal memory access|Memory access fault|HSA_STATUS_ERROR|GPU hang", re.I)


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    from m4ri_rust_amd import device
    device.require_gpu()
    return p


def run_child(case, setting, timeout=120):
    """-> (stdout, stderr) of a fresh process that ran switch_child.run(case) under `setting`; fails the test unless it ended with SWITCH-OK"""
    global _crashed
    if _crashed:
        pytest.skip("not started: an earlier child process of this file crashed (%s)" % _crashed)
    script = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
              "import switch_child\n"
              "switch_child.run(%r)\n") % (ROOT, os.path.join(ROOT, "tests"), case)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}  # only the case's own setting
    env.update({k: str(v) for k, v in setting.items()})
    what = "%s under %s" % (case, setting)
    try:
        r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        _crashed = "%s did not end within %d s" % (what, timeout)
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(_crashed + "\n" + out[-1500:] + err[-3000:])
    tail = r.stdout[-1500:] + r.stderr[-3000:]
    if r.returncode < 0 or r.returncode in (134, 139) or (r.returncode != 0 and DEVICE_TROUBLE.search(r.stdout + r.stderr)):
        _crashed = "%s ended with status %d" % (what, r.returncode)
        pytest.fail(_crashed + "\n" + tail)
    assert r.returncode == 0 and ("SWITCH-OK " + case) in r.stdout, what + "\n" + tail
    return r.stdout, r.stderr


def plans_of(stdout):
    line = [ln for ln in stdout.splitlines() if ln.startswith("SWITCH-PLANS ")][-1]
    return json.loads(line[len("SWITCH-PLANS "):])


@pytest.mark.parametrize("cfg", [7, 8, 9, 10, 11, 12, 20, 81, 82])
def test_forced_tile_variant(pkg, cfg):
    """M4RI_HIP_M4RM_CFG, how every A/B run of the tile kernel is made: through the planner and the launcher (plan_tiles, apply_tile_plan,
    the refusal of packed operands by the older variants), plain products ragged everywhere / with a ragged last tile row / with a long
    inner dimension / of a shape whose default plan packs A, and Strassen leaf batches (one level, two levels, a padded plan)."""
    run_child("cfg", {"M4RI_HIP_M4RM_CFG": cfg})


def test_tile_variant_outside_the_accepted_list(pkg):
    """M4RI_HIP_M4RM_CFG=5: ignored with a message; plans and bits are the default's"""
    out, err = run_child("cfg_ignored", {"M4RI_HIP_M4RM_CFG": 5})
    assert "M4RI_HIP_M4RM_CFG=5 ignored" in err, err[-1500:]
    import switch_child  # (this process has no M4RI_HIP_M4RM_CFG: its answers are the default's)
    assert "M4RI_HIP_M4RM_CFG" not in os.environ
    assert plans_of(out) == json.loads(json.dumps(switch_child.plans_of_every_shape(), sort_keys=True))


def test_strassen_leaves_row_major(pkg):
    """M4RI_HIP_APACK=0: the leaf batches of the three Strassen shapes and the 343 leaves of 2048^3 with three levels, unpacked"""
    run_child("apack0", {"M4RI_HIP_APACK": 0})


def test_plain_products_never_pack(pkg):
    """M4RI_HIP_PLAIN_APACK=0 at 1024 x 1024 x 70000 (whose default plan packs A) and 4608 x 1024 x 1024"""
    run_child("plain_apack0", {"M4RI_HIP_PLAIN_APACK": 0})


@pytest.mark.parametrize("mib", [0, 1])
def test_no_scratch_for_partial_tiles(pkg, mib):
    """M4RI_HIP_SPLITK_WS_MIB = 0 / 1: whole unsplit tiles for the four plain shapes; automatic Strassen levels at 4096^3, padded plans at
    4100^3 and 5000 x 4000 x 4100"""
    run_child("splitk_ws", {"M4RI_HIP_SPLITK_WS_MIB": mib})


@pytest.mark.parametrize("mib", [0, 1])
@pytest.mark.parametrize("cfg", [8, 7])
def test_no_scratch_for_a_forced_split_k_variant(pkg, cfg, mib):
    """M4RI_HIP_SPLITK_WS_MIB = 0 / 1 with a forced v6 / v3 variant: the launch runs unsplit and the plan query says so (600 x 4096 x 600,
    the leaves of 4096^3)"""
    run_child("splitk_ws_cfg", {"M4RI_HIP_SPLITK_WS_MIB": mib, "M4RI_HIP_M4RM_CFG": cfg})


@pytest.mark.parametrize("leaf_min", [512, 4096])
def test_strassen_leaf_min(pkg, leaf_min):
    """M4RI_HIP_STRASSEN_LEAF_MIN (with M4RI_HIP_SPLITK_WS_MIB=1, under which levels pay at small shapes): 512 gives two levels at 2048^3
    and a padded one-level plan at 3000^3; 4096 keeps 4096^3 plain"""
    run_child("leaf_min_%d" % leaf_min, {"M4RI_HIP_SPLITK_WS_MIB": 1, "M4RI_HIP_STRASSEN_LEAF_MIN": leaf_min})


@pytest.mark.parametrize("max_levels", [1, 0])
def test_strassen_max_levels(pkg, max_levels):
    """M4RI_HIP_STRASSEN_MAX_LEVELS caps the automatic choice (one level at 2048^3 where two were chosen; none at 4096^3); an explicit
    level count is honoured as given"""
    setting = {"M4RI_HIP_SPLITK_WS_MIB": 1, "M4RI_HIP_STRASSEN_MAX_LEVELS": max_levels}
    if max_levels == 1:
        setting["M4RI_HIP_STRASSEN_LEAF_MIN"] = 512
    run_child("max_levels_%d" % max_levels, setting)


@pytest.mark.parametrize("setting", [{"M4RI_HIP_STRASSEN_PAD": 0}, {"M4RI_HIP_STRASSEN_PAD": 0, "M4RI_HIP_SPLITK_WS_MIB": 1}],
                         ids=["alone", "where the automatic choice would pad"])
def test_strassen_padding_switched_off(pkg, setting):
    """M4RI_HIP_STRASSEN_PAD=0: 1030 x 2049 x 2050 with one level asked for and 5000 x 4000 x 4100 automatic run as given (kind 0, the levels
    the level choice alone gives: none), so neither the padding copy nor a split / merge pass launches; bits against the oracle"""
    run_child("pad0", setting)


@pytest.mark.parametrize("blocks", [1, 2, 8])
def test_host_pipeline_blocks(pkg, blocks):
    """M4RI_HIP_HOST_PIPELINE_BLOCKS through mzd_mul_m4rm / mzd_mul_naive on host matrices, the thin pipeline's shape (65536 x 1024 x 64).
    No observable of the block count exists: bits only."""
    run_child("pipeline_blocks", {"M4RI_HIP_HOST_PIPELINE_BLOCKS": blocks})


def test_host_pipeline_two_blocks_big(pkg):
    """16384^3 on host matrices in two row blocks, about 200 sampled rows against the oracle.  Bits only."""
    run_child("pipeline_big", {"M4RI_HIP_HOST_PIPELINE_BLOCKS": 2}, timeout=300)


def test_every_host_transpose_on_the_device(pkg):
    """M4RI_HIP_TRANSPOSE_GPU_MIN_BITS=1: mzd_transpose of 1 x 1 ... 129 x 300 through the device kernel (NULL and plain destinations, a
    source window of a dirty parent) and through the host loop (a destination window)"""
    run_child("transpose", {"M4RI_HIP_TRANSPOSE_GPU_MIN_BITS": 1})


@pytest.mark.parametrize("setting", [{"M4RI_HIP_PIN_MIN_BYTES": 4096}, {"M4RI_HIP_PIN_MIN_BYTES": 1 << 40}, {"M4RI_HIP_PIN_CACHE_BYTES": 0}],
                         ids=["pinned from 4 KiB", "never pinned", "no pinned blocks kept"])
def test_pinned_host_blocks(pkg, setting):
    """A * v (2^18 x 256 x 1 through mul_slice, x 3 through mzd_mul_naive), 16384 x 256 x 64, and mzd_init after mzd_free of a filled
    2 MiB matrix.  No public observable of pinning exists: bits only."""
    run_child("pinning", setting)
