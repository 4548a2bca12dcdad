"""CPU: the host shim under AddressSanitizer + UndefinedBehaviorSanitizer (SURVEY.md §5 "race detection / sanitizers";
round-5 verdict, item 7: lbl_api.hip is 2,500 lines of pools, caches, registries, views and schedule builders behind raw
pointers and no sanitizer had ever seen it).

tests/host_shim/ builds pyrad_amd/csrc/lbl_api.hip - unchanged, as plain C++ - against a stand-in HIP runtime whose
"device" memory is host memory (mock/hip/hip_runtime.h) and launchers that read and write exactly the index ranges the
kernels read and write (mock_kernels.cpp, sharing the launch-shape arithmetic of pyrad_amd/csrc/lbl_launch_shapes.h with the
real launchers), with -fsanitize=address,undefined and scratch blocks without slack (-DLBL_SANITIZER_BUILD).  shim_driver
then goes through the PUBLIC C ABI with seeded random cells, shards, columns, 70-line-list layers, views, option
settings, graph captures, bad arguments, injected allocation failures and random destruction orders; every object the
stand-in runtime handed out must have come back at the end.

The stand-in runtime copies synchronously, so by itself it cannot see a page-locked staging block that the host rewrites before
a queued hipMemcpyAsync has read it.  It therefore keeps the source range of every staged host-to-device copy poisoned until the
host has waited for something that covers the copy (mock/hip/hip_runtime.h), and the driver opens with a run of column sweeps that
stages four laps of the 8-block staging ring without a stream synchronisation in between (stage_alloc once took the half it was
leaving from the END of the last allocation: a block ending exactly on the middle of the ring recorded no event, and nothing was
ever waited for).  CPU only: nothing of this is ever linked into
libpyrad_hip.so or run on the GPU box."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

DIR = os.path.join(REPO, "tests", "host_shim")
BIN = os.path.join(DIR, "_build", "shim_driver")


@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None:
        pytest.skip("no g++ for the sanitizer build")
    p = subprocess.run(["make", "-C", DIR], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return BIN


def run(driver, seed, rounds, env_extra=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.update(env_extra or {})
    return subprocess.run([driver, str(seed), str(rounds)], capture_output=True, text=True, env=env, timeout=600)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_random_abi_sequences_are_clean_under_asan_and_ubsan(driver, seed):
    p = run(driver, seed, 12)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-6000:])
    assert "no sanitizer report, nothing leaked" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr


def test_the_harness_sees_a_block_sized_too_small(driver):
    """self-test: the line-prep stand-in made to write counters past what the shim reserved for them is reported"""
    p = run(driver, 1, 3, {"SHIM_INJECT_OVERRUN": "1"})
    assert p.returncode != 0 and "AddressSanitizer" in p.stderr and "buffer-overflow" in p.stderr


def test_the_staging_ring_run_reaches_the_boundary_and_is_clean(driver):
    """the run of column sweeps stages 8 + 32 blocks of one size: blocks end on the middle of the pinned ring and ranges are written
    again after a copy out of them (so it cannot pass by never getting there), and no block is written while a copy is pending"""
    p = run(driver, 1, 1)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-6000:])
    m = re.search(r"staging ring run: (\d+) staged copies, (\d+) ended on the middle of their pinned block, (\d+) out of a range written again", p.stdout)
    assert m, p.stdout[-500:]
    copies, on_middle, rewrites = (int(x) for x in m.groups())
    assert copies >= 8 + 17 and on_middle >= 2 and rewrites >= 2, m.group(0)


def test_the_harness_sees_a_pinned_block_written_before_its_copy_was_waited_for(driver):
    """self-test: with the stand-in's hipEventSynchronize covering nothing (as if the ring had not waited for the half it enters)
    the same run is reported as a write into a poisoned range"""
    p = run(driver, 1, 1, {"SHIM_INJECT_NO_EVENT_WAIT": "1"})
    assert p.returncode != 0 and "AddressSanitizer" in p.stderr and "use-after-poison" in p.stderr
    assert re.search(r"^\s*#\d+ 0x[0-9a-f]+ in (device_args|stage_alloc)\b", p.stderr, re.M), p.stderr[:3000]      # a frame of the report's stack
