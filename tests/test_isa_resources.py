"""CPU: the gate over EVERY unit the library ships (round-4 review: launched kernels spilled, nothing noticed), one case per entry of
the manifest build.UNITS.  A kernel unit's code object metadata is read (what the loader goes by) and held to the floor and to its
entry of the gate table, tests/unit_gates.py, which states the rules; a host or cpp unit holds no device code and stays small.
Manifest, gate table and csrc/ must name the same units, so a unit cannot be added without its gate."""
import os
import re
import subprocess

import pytest

import isa_tools as T
import unit_gates as UG
from rgbd_pose_estimation_amd import build as B

KIND = {src: kind for src, kind, _ in B.UNITS}


def check_kernel_unit(unit, rows):
    """the floor and the unit's gate entry over the kernels `rows` of the unit"""
    assert unit in UG.GATES, f"{unit} is a kernel unit of build.UNITS without an entry in tests/unit_gates.py GATES"
    gate = UG.GATES[unit]
    floor = dict(UG.FLOOR, scratch=UG.PRIVATE_ARRAYS.get(unit, UG.FLOOR["scratch"]))
    limit = dict(floor, **{k: v for k, v in gate.items() if k in ("sgpr_spill", "scratch", "regs")})
    assert all(limit[k] <= floor[k] for k in floor), (unit, limit)       # an entry tightens the floor, never loosens it
    assert rows, unit
    if "kernels" in gate:
        assert T.kernel_bases(UG.obj(unit)) == gate["kernels"]
    for key in ("vgpr_spill", "sgpr_spill", "scratch"):
        if key in limit:
            over = [(r["name"], r[key]) for r in rows if r[key] > limit[key]]
            assert not over, (key, over[:10])
    over = [(r["name"], r["vgpr"], r["agpr"]) for r in rows if r["vgpr"] + r["agpr"] > limit["regs"]]
    assert not over, over[:10]
    lds = gate.get("lds", {})
    assert set(lds) <= set(gate.get("kernels", {})) | {"*"}, lds
    for r in rows:
        for lo, hi in (lds[k] for k in ("*", r["base"]) if k in lds):
            assert lo <= r["lds"] <= hi, (r["name"], r["lds"], lo, hi)
    # the unit names its own preload kernel: RPE_PRELOAD's node, built by the constructor in rpe_context.hip, and no function of its own
    syms = subprocess.check_output(["nm", "-C", UG.obj(unit)]).decode()
    assert re.search(r"^\s+U rpe::PreloadNode::PreloadNode\(void const\*\)$", syms, re.M) and "preload_" not in syms, unit


@pytest.mark.parametrize("unit", B.SOURCES, ids=[os.path.splitext(u)[0] for u in B.SOURCES])
def test_no_kernel_spills_and_none_carries_scratch(unit):
    """the gate of one unit of the manifest, whatever its kind: a host or cpp unit passes by holding no kernel at all"""
    UG.built()
    assert unit in B.__doc__ and os.path.exists(os.path.join(UG.CSRC, unit))
    rows = T.kernel_resources(UG.obj(unit))
    if KIND[unit] == "kernel":
        return check_kernel_unit(unit, rows)
    assert KIND[unit] in ("host", "cpp") and rows == [], unit
    if KIND[unit] == "host":
        assert os.path.getsize(os.path.join(UG.CSRC, unit)) < UG.MAX_HOST_SOURCE_BYTES, unit
        comment = open(os.path.join(UG.CSRC, "rpe_host.hpp")).read().split("#pragma once")[0]
        assert f"//   {unit} " in comment, unit


def test_manifest_gate_table_and_sources_name_the_same_units():
    assert len(set(B.SOURCES)) == len(B.SOURCES) == len(B.UNITS)
    assert set(B.SOURCES) == {f for f in os.listdir(UG.CSRC) if f.endswith((".hip", ".cpp"))}
    assert set(UG.GATES) == {u for u, k in KIND.items() if k == "kernel"}
    assert set(UG.PRIVATE_ARRAYS) | set(UG.MAX_KERNELS) <= set(UG.GATES)


def test_kernel_counts_and_library_size():
    so = UG.built()
    counts = {u: len(T.kernel_resources(UG.obj(u))) for u in UG.MAX_KERNELS}
    assert all(counts[u] <= UG.MAX_KERNELS[u] for u in counts), counts
    assert os.path.getsize(so) < UG.MAX_LIBRARY_BYTES, os.path.getsize(so)


def test_no_host_unit_outgrows_its_job():
    """the headers the host units share; the units themselves are held to the same size by the gate above"""
    for u in UG.SHARED_HOST_HEADERS:
        assert os.path.getsize(os.path.join(UG.CSRC, u)) < UG.MAX_HOST_SOURCE_BYTES, u
