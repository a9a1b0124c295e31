"""csrc/batch_buffers.hpp -- the owning buffers and the pinned slot ring of a batch's state -- as host code: the header is built with
tests/host_kernels/batch_buffers_main.cpp as a stand-alone program (g++ -std=c++17 -O1 -g -fsanitize=address,undefined
-fno-sanitize-recover=undefined) against ROCm's runtime header; the program defines the nine runtime calls the header makes as fakes
over malloc that log themselves, and runs as a child process.  Nothing is loaded into python and nothing runs on a GPU.

What is read off the log: every growth waits for the stream, then frees, then allocates; a grow that fits makes no call; a failed
allocation leaves an empty buffer that a later grow serves; nothing is left live and nothing is freed twice (the fakes abort on a free
of a block that is not live, AddressSanitizer on anything the fakes miss); the ring hands out slots 0, 1, 2, 3, 0, ... and waits on a
slot's own event from its second use on; a growth restarts the count and creates no second set of events."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SLOTS = 4
CALLS = ("sync", "malloc", "free", "event_create", "event_destroy", "event_sync", "event_record")


@pytest.fixture(scope="module")
def log(tmp_path_factory):
    """{scenario: [line]} of the program's one run."""
    d = str(tmp_path_factory.mktemp("batch_buffers_host"))
    exe = os.path.join(d, "batch_buffers_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(ROCM, "include"), "-I", CSRC, os.path.join(HERE, "batch_buffers_main.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr.strip() == "", p.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stderr == "", "exit %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])      # (the sanitizers are silent)
    out = {}
    for line in p.stdout.splitlines():
        if line.startswith("scenario "):
            out[line.split()[1]] = cur = []
        else:
            cur.append(line)
    return out


def calls(lines):
    return [l for l in lines if l.split()[0] in CALLS]


def between(lines, start, stop=None):
    """The lines after the first `start` up to the next line that starts with `stop` (or the end)."""
    i = lines.index(start) + 1
    j = next((k for k in range(i, len(lines)) if stop is not None and lines[k].startswith(stop)), len(lines))
    return lines[i:j]


def test_the_header_includes_the_runtime_api_and_the_standard_library_only():
    text = open(os.path.join(CSRC, "batch_buffers.hpp")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes[0] == "<hip/hip_runtime_api.h>" and all(i.startswith("<c") and i.endswith(">") for i in includes[1:]), includes
    for word in ("cpprob_hip_ctx", "HIP_TRY", "fail("):
        assert word not in text
    assert "= delete" in text and "hipHostMallocDefault" in text and "hipEventDisableTiming" in text


@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_a_buffer_waits_then_frees_then_allocates_and_leaves_nothing(log, kind):
    L = log[kind]
    assert L[0] == "state null 1 capacity 0"
    # a grow of 0 bytes and every grow that fits: no call, grew = 0, the state unchanged
    assert L[1] == "grow 0 -> 0 grew 0"
    assert L[2:5] == ["sync", "malloc %s 100" % kind, "grow 100 -> 0 grew 1"]              # (nothing to free yet; it waits all the same)
    assert L[5:8] == ["state null 0 capacity 100", "grow 100 -> 0 grew 0", "grow 7 -> 0 grew 0"]
    # the second growth: the wait, then the free, then the allocation
    assert L[8:13] == ["sync", "free %s" % kind, "malloc %s 101" % kind, "grow 101 -> 0 grew 1", "state null 0 capacity 101"]
    assert between(L, "release", "destroy") == ["free %s" % kind, "state null 1 capacity 0", "sync", "malloc %s 5" % kind, "grow 5 -> 0 grew 1"]
    assert between(L, "destroy") == ["free %s" % kind, "live device 0 pinned 0 events 0"]
    c = calls(L)
    assert len([x for x in c if x.startswith("malloc")]) == len([x for x in c if x.startswith("free")]) == 3
    for i, x in enumerate(c):                   # every allocation: the call before it is the wait or the free, and a free of a growth follows the wait
        if x.startswith("malloc"):
            assert c[i - 1] == "sync" or (c[i - 1].startswith("free") and c[i - 2] == "sync")


@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_a_failed_allocation_leaves_an_empty_buffer_that_grows_again(log, kind):
    L = log[kind + "_failure"]
    assert L[:3] == ["sync", "malloc %s 64" % kind, "grow 64 -> 0 grew 1"]
    # the growth that fails: waited, freed, refused -- and told as a growth, the old block is gone; then null and 0 (not the pointer the
    # failed call left), nothing live
    assert L[3:9] == ["sync", "free %s" % kind, "malloc %s 128 failed" % kind, "grow 128 -> 1 grew 1", "state null 1 capacity 0", "live device 0 pinned 0 events 0"]
    assert L[9:13] == ["sync", "malloc %s 32" % kind, "grow 32 -> 0 grew 1", "state null 0 capacity 32"]      # (no free of the block that never was)
    assert L[13:17] == ["sync", "free %s" % kind, "malloc %s 256 failed" % kind, "grow 256 -> 1 grew 1"]
    assert between(L, "destroy") == ["live device 0 pinned 0 events 0"]                 # (the destructor of an empty buffer makes no call)


def uses(lines):
    """[(slot, count before, [calls of the use])] of the ring's uses in `lines`."""
    out, cur = [], []
    for l in lines:
        if l.startswith("slot "):
            w = l.split()
            assert w[5] == "0"
            out.append([int(w[1]), int(w[3]), cur])
            cur = []
        elif l.startswith("commit"):
            assert l == "commit -> 0"
            out[-1][2] = out[-1][2] + cur
            cur = []
        elif l.split()[0] in CALLS:
            cur.append(l)
    return out


def test_the_ring_hands_out_its_slots_in_turn_and_waits_on_a_slots_own_event(log):
    L = log["ring"]
    # the first reserve: the block of SLOTS slots (waited for like any growth), then the events, once
    assert L[:3 + SLOTS] == ["sync", "malloc pinned %d" % (SLOTS * 48)] + ["event_create %d" % i for i in range(SLOTS)] + ["reserve 48 -> 0 grew 1 stride 48 count 0"]
    first = uses(between(L, "reserve 48 -> 0 grew 1 stride 48 count 0", "uncommitted"))
    assert [u[0] for u in first] == [i % SLOTS for i in range(10)] and [u[1] for u in first] == list(range(10))
    for i, (slot, _, c) in enumerate(first):    # no wait in the first SLOTS uses; from use SLOTS + 1 on, the slot's own event alone, before its record
        assert c == (["event_sync %d" % slot] if i >= SLOTS else []) + ["event_record %d" % slot]
    # an acquire without a commit hands out the same slot again, and records nothing
    again = uses(between(L, "uncommitted", "reserve"))
    assert [(u[0], u[1]) for u in again] == [(2, 10)] * 3
    assert [u[2] for u in again] == [["event_sync 2"], ["event_sync 2"], ["event_sync 2", "event_record 2"]]
    # a reserve that fits (the same stride, a smaller one): no call, the count goes on
    assert between(L, "reserve 48 -> 0 grew 0 stride 48 count 11", "reserve 80")[:-3] == ["reserve 16 -> 0 grew 0 stride 48 count 11"]
    assert L[L.index("reserve 48 -> 0 grew 0 stride 48 count 11") - 1] == "commit -> 0"
    # a growth: waited, freed, allocated; the count starts again; no second set of events
    i = L.index("reserve 80 -> 0 grew 1 stride 80 count 0")
    assert L[i - 3:i] == ["sync", "free pinned", "malloc pinned %d" % (SLOTS * 80)]
    grown = uses(between(L, "reserve 80 -> 0 grew 1 stride 80 count 0", "restart"))
    assert [(u[0], u[1]) for u in grown] == [(j % SLOTS, j) for j in range(6)]
    assert [u[2] for u in grown] == [(["event_sync %d" % (j % SLOTS)] if j >= SLOTS else []) + ["event_record %d" % (j % SLOTS)] for j in range(6)]
    # restart: the count is 0 again and the first SLOTS uses wait for nothing
    re = uses(between(L, "restart", "reserve 81"))
    assert [(u[0], u[1]) for u in re] == [(j % SLOTS, j) for j in range(5)] and [len(u[2]) for u in re] == [1, 1, 1, 1, 2]
    assert "reserve 81 -> 0 grew 1 stride 81 count 0" in L
    assert len([l for l in L if l.startswith("event_create")]) == SLOTS
    # destruction: every event once, then the block
    assert between(L, "destroy") == ["event_destroy %d" % j for j in range(SLOTS)] + ["free pinned", "live device 0 pinned 0 events 0"]
    assert len([l for l in L if l.startswith("malloc")]) == len([l for l in L if l.startswith("free")]) == 3


def test_a_ring_whose_block_fails_to_grow_serves_no_slot_until_it_has_grown(log):
    L = log["ring_failure"]
    assert L[:4] == ["sync", "malloc pinned %d failed" % (SLOTS * 32), "reserve 32 -> 1 grew 1 stride 0 count 0", "live device 0 pinned 0 events 0"]
    i = L.index("reserve 32 -> 0 grew 1 stride 32 count 0")
    assert L[4:i] == ["sync", "malloc pinned %d" % (SLOTS * 32)] + ["event_create %d" % (SLOTS + j) for j in range(SLOTS)]
    # a growth that fails after a use: the stride and the count are 0, and the next reserve -- of any size -- allocates afresh
    j = L.index("reserve 64 -> 1 grew 1 stride 0 count 0")
    assert L[j - 3:j] == ["sync", "free pinned", "malloc pinned %d failed" % (SLOTS * 64)]
    assert L[j + 1:j + 4] == ["sync", "malloc pinned %d" % (SLOTS * 8), "reserve 8 -> 0 grew 1 stride 8 count 0"]
    assert [(u[0], u[1]) for u in uses(L[j + 4:L.index("destroy")])] == [(0, 0)]
    assert between(L, "destroy") == ["event_destroy %d" % (SLOTS + k) for k in range(SLOTS)] + ["free pinned", "live device 0 pinned 0 events 0"]
    assert len([l for l in L if l.startswith("event_create")]) == SLOTS


def test_what_was_never_grown_is_destroyed_without_a_call(log):
    assert log["untouched"] == ["destroy", "live device 0 pinned 0 events 0"]
