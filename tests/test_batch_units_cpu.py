"""Which bucket-split MSMs of one call run as ONE launch per pipeline stage -- msel::batch_units in accumulation_amd/csrc/msm_select.h --
at every edge, without a GPU: tests/cpp_host/batch_units_check.cpp is plain C++ over the header alone (it exits non-zero when a unit
list does not cover its jobs exactly once in order, when a unit holds jobs that differ, or when a unit's tail is not covered by what
the plan reserves before the Place is known: the fixture's check=True).  The expected unit lists live here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_host", "batch_units_check.cpp")
EXE = os.path.join(ROOT, "build", "batch_units_check")


@pytest.fixture(scope="module")
def lines():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", EXE])
    out = subprocess.run([EXE], capture_output=True, text=True, check=True).stdout.splitlines()
    units = {w[1]: w[2] for w in (ln.split() for ln in out) if w[0] == "units"}
    tails = [ln.split() for ln in out if ln.startswith("unit_tail ")]
    return units, tails


def test_runs_are_cut_into_units_of_up_to_eight(lines):
    units, _ = lines
    assert [units[f"run_{k}"] for k in (0, 1, 2, 8, 9, 17)] == ["-", "1", "2", "8", "8+1", "8+8+1"]
    assert units["two_runs"] == "3+3"


@pytest.mark.parametrize("field", ["n", "off", "mont", "skip_ones", "force_chunked", "key", "grouped", "shared", "no_geom", "empty"])
def test_a_job_that_differs_splits_the_run(lines, field):
    assert lines[0][f"mid_{field}"] == "2+1+2"


def test_grouped_and_shared_jobs_never_join_a_unit(lines):
    units, _ = lines
    assert units["all_grouped"] == units["all_shared"] == "1+1+1+1"


def test_the_switches(lines):
    units, _ = lines
    assert units["cap_0"] == units["cap_1"] == "+".join(["1"] * 7)
    assert (units["cap_2"], units["cap_3"], units["cap_8"]) == ("2+2+2+1", "3+3+1", "7")
    assert units["bps_0"] == units["bps_1"] == units["window_override"] == "1+1+1+1"  # nothing takes the pipeline: nothing to batch


def test_a_unit_stays_below_512_mib_of_its_slot(lines):
    units, _ = lines
    want = {64: "8", 65: "7+1", 128: "4+4", 200: "2+2+2+2", 256: "2+2+2+2", 257: "+".join(["1"] * 8), 600: "+".join(["1"] * 8)}
    assert {m: units[f"slot_{m}_mib"] for m in want} == want


def test_only_bucket_split_sizes_and_keys_form_units(lines):
    units, _ = lines
    assert [units[f"pairs_{n}"] for n in ((1 << 16) - 1, 1 << 16, 1 << 17, (1 << 17) + 1)] == ["1+1+1", "3", "3", "1+1+1"]
    assert (units["key_bpl_over_twin"], units["key_plain"], units["key_direct"]) == ("3", "1+1+1", "1+1+1")


def test_a_units_tail_is_covered_at_every_place(lines):
    _, tails = lines
    assert len(tails) == 3 * 7 * 3  # three geometries, V = 2 .. 8, three places
    assert all(t[-1] == "covered=1" for t in tails)
    # an exposed tail is the fused quad form whatever the unit's size; a hidden one takes it while the unit's bucket table is small
    assert all(t[3] == "form=fused_quad" for t in tails if t[2] in ("lone", "batch_last"))
    hidden = {t[1]: t[3] for t in tails if t[2] == "batch_inner"}
    assert hidden["w16_2p16_x4"] == "form=fused_quad" and hidden["w16_2p16_x5"] == "form=one_lane"
