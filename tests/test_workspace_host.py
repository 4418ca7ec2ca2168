"""The shared pieces of the device workspaces (indy-plenum_amd/csrc/workspace.h and stage.h: grow-only device and
pinned buffers, the owner of a context's resources, the event hand-over between caller streams, the
256-byte staging layout, the offsets check, the staged call of a host-buffer entry, the path choice), compiled with g++ against a stub HIP runtime
(tests/native/stub_hip) that logs every call and can fail a creation, a copy or a synchronisation. Built with AddressSanitizer and UBSan and run as a stand-alone program. CPU only."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "workspace_check.cpp")
STUB = os.path.join(HERE, "native", "stub_hip")
HDR = os.path.join(HERE, "..", "indy-plenum_amd", "csrc", "workspace.h")
STAGE_HDR = os.path.join(HERE, "..", "indy-plenum_amd", "csrc", "stage.h")
BIN = os.path.join(HERE, "native", "workspace_check")


@pytest.fixture(scope="module")
def report():
    deps = [SRC, HDR, STAGE_HDR, os.path.join(STUB, "hip", "hip_runtime.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", STUB, "-o", BIN, SRC])
    out = subprocess.run([BIN], check=True, capture_output=True, text=True, timeout=60).stdout
    return json.loads(out)


def _group(report, name, at_least):
    checks = {k: v for k, v in report.items() if k.startswith(name + ".")}
    assert len(checks) >= at_least, sorted(checks)
    assert all(v is True for v in checks.values()), {k: v for k, v in checks.items() if v is not True}


def test_device_buffer_is_empty_after_a_failed_grow(report):
    """grow(want <= cap) makes no runtime call; a failed grow returns PV_ERR_ALLOC and leaves p == nullptr
    and cap == 0, so the next grow of any size allocates again; release twice is harmless; allocations
    equal frees."""
    _group(report, "dev", 13)


def test_pinned_buffer_is_empty_after_a_failed_grow(report):
    """The same for pinned memory, and the hipHostMalloc flags arrive unchanged."""
    _group(report, "pinned", 13)


def test_hand_over_waits_only_for_another_stream(report):
    """Read from the stub's call log: no wait on the first use or on the stream that used the workspace
    last, exactly one wait (on the waiting stream, for the recorded event) otherwise; a forgotten stream is
    never waited for; destroy, then begin, recreates the event."""
    _group(report, "hand", 15)


def test_owner_releases_what_it_created_however_far_creation_got(report):
    """PvOwner over 3 streams, 4 events, 6 device and 2 pinned blocks created interleaved as an engine context
    creates them: sizes, flags and the priority reach the runtime unchanged; release_all balances every kind,
    newest first, and a second one makes no call; drop frees one block once; with creation k failing, for
    every k, that call returns its error code with a null out-parameter and one release_all leaves nothing
    behind (the half-built context no GPU test can reach); an optional pair whose second half fails leaves
    the owner as it was."""
    _group(report, "owner", 19)


def test_stage_lays_out_rebases_copies_and_recovers_in_both_modes(report):
    """PvStage in caller-memory and in pinned mode over the stub's malloc-backed blocks: sections are 256-byte
    aligned, disjoint, inside their block and non-null when empty; offsets that start at 37 arrive starting at
    0 and the caller's array is untouched; slack is reserved and never read from the caller; outputs arrive
    byte for byte, a null dst is skipped, an arena goes up and comes back; the log holds one copy per
    non-empty section (caller memory) or one up and one down (pinned) and one synchronise; a larger chunk
    grows the blocks and smaller ones allocate nothing; with each grow, each copy and the synchronise failing
    in turn the use returns PV_ERR_ALLOC / PV_ERR_LAUNCH, and the next use synchronises before its first copy
    and succeeds; a lent array survives later sections; the AUTO / HOST / DEVICE choice over its whole table,
    error text included."""
    _group(report, "stage", 2 * 21 + 4)
    assert sum(k.startswith("stage.caller_") for k in report) == sum(k.startswith("stage.pinned_") for k in report)


def test_layout_sections_are_aligned_and_disjoint(report):
    _group(report, "layout", 5)


def test_offsets_monotone(report):
    _group(report, "monotone", 6)
