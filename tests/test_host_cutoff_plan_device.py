"""The element-by-element rules of the device-side build of the cutoff plan (csrc/kmvp_cutoff_plan_device.hpp; "cutoff_plan"
= 1 of include/kmvp.h) without a GPU: tests/host_cutoff_plan_device_shim.cpp runs the very functions the kernels of
csrc/kmvp_cutoff_plan_device.hip call -- a stable sort for the radix sort, serial loops for the scans, one trip per thread --
and every plan must equal cutoff_plan_build's on the same input entry for entry, the numpy restatement's
(cutoff_reference.plan) as well, and have the properties the pair-loop kernels rely on (test_host_cutoff_plan.py
check_properties): the kernels index the tables without a bounds check."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import cutoff_plan_cases as cases
import cutoff_reference as cr
import test_host_cutoff_plan as host

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")
PREC = {"f32": np.float32, "f64": np.float64}


class HostBuild:
    """The shim's library with hc_build answered by cutoff_plan_build: what test_host_cutoff_plan.build() reads."""

    def __init__(self, lib):
        self._lib = lib
        self.hc_build = lib.hd_build_host

    def __getattr__(self, name):
        return getattr(self._lib, name)


@pytest.fixture(scope="module")
def lib():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_cutoff_plan_device_")
    so = os.path.join(tmp, "libhost_cutoff_plan_device.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_cutoff_plan_device_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    for fn in (lib.hc_build, lib.hd_build_host):
        fn.restype = ctypes.c_void_p
        fn.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    lib.hc_free.restype = None
    lib.hc_free.argtypes = [ctypes.c_void_p]
    for fn, n in ((lib.hc_sizes, 3), (lib.hc_tables, 3), (lib.hc_maps, 3)):
        fn.restype = None
        fn.argtypes = [ctypes.c_void_p] * n
    lib.hd_fits.argtypes = [ctypes.c_longlong] * 3
    lib.hd_key_bits.argtypes = [ctypes.c_longlong]
    lib.hd_bounds.restype = None
    lib.hd_bounds.argtypes = [ctypes.c_longlong] * 3 + [ctypes.c_int, ctypes.c_void_p]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def check(lib, y, x, R, factor):
    got = host.build(lib, y, x, R, factor)
    cases.equal_plans(got, host.build(HostBuild(lib), y, x, R, factor))
    cases.equal_plans(got, cr.plan(y, y if x is None else x, R, factor))
    host.check_properties(got, y, x, R, factor)
    # what the device build allocates for holds the plan
    bounds = np.zeros(3, dtype=np.int64)
    lib.hd_bounds(len(y if x is None else x), len(y), int(got["g"][1] * got["g"][2]), y.shape[1], bounds.ctypes.data)
    assert len(got["tiles"]) <= bounds[0] and len(got["runs"]) <= bounds[1] and got["m_alloc"] <= bounds[2]
    return got


@pytest.mark.parametrize("prec", list(PREC))
def test_every_case_equals_the_host_build(lib, prec):
    seen = {}
    for name, y, x, R, factor in cases.cases(PREC[prec]):
        seen[name] = check(lib, y, x, R, factor)
    # the cases are what their names say
    assert list(seen["cloud C x1.0"]["tiles"][:3, 2]) == [64, 64, 2]
    assert sorted(seen["rows of 64 and 65"]["tiles"][:4, 2]) == [1, 7, 64, 64] and seen["rows of 64 and 65"]["live_tiles"] == 4
    p = seen["130 loose targets"]
    assert list(p["tiles"][p["live_tiles"] - 3:p["live_tiles"], 2]) == [64, 64, 2] and np.all(p["tiles"][p["live_tiles"] - 3:, 1] == 0)
    assert np.all(np.diff(p["tmap"][(p["live_tiles"] - 3) * cr.TILE:][:130]) > 0)       # the loose targets in the caller's order
    p = seen["identical points"]
    assert np.any(np.all(p["tmap"].reshape(-1, cr.TILE)[:, [0, -1]] >= 30, axis=1) & np.all(p["tmap"].reshape(-1, cr.TILE)[:, [0, -1]] < 180, axis=1))
    assert seen["all sources non-finite"]["m_pad"] == 0 and len(seen["all sources non-finite"]["runs"]) == 0
    assert seen["everything non-finite"]["live_tiles"] == 2 and np.all(seen["everything non-finite"]["g"] == 1)
    assert seen["M = 0"]["m_alloc"] == cr.RECORDS and seen["N = 0"]["n_pad"] == 0
    assert np.all(seen["one cell"]["g"] == 1) and seen["one cell"]["walked"] == 70 * 104
    assert seen["cell cap"]["h"] > 2e-9 and int(np.prod(seen["cell cap"]["g"])) <= 200
    assert any(p["live_tiles"] % cr.WAVES for p in seen.values())
    assert int(np.prod(seen["clustered"]["g"])) > 4 * len(np.unique(seen["clustered"]["runs"][:, 0]))    # mostly empty cells


def test_same_points_and_a_copy_agree(lib):
    """Targets = sources shares one sorted cloud; a separate copy of the same points sorts twice.  Same plan."""
    y = np.random.RandomState(0).rand(500, 3)
    cases.equal_plans(host.build(lib, y, None, 0.2, 1.0), host.build(lib, y, y.copy(), 0.2, 1.0))


def test_fits_in_32_bits(lib):
    top = 2 ** 31 - 1
    assert lib.hd_fits(top, top, 5) == 1 and lib.hd_fits(5, top, top - 1) == 1
    # ... and the longest scan has one entry per tile the table may hold, a partial tile per row included
    assert lib.hd_fits(top, 5, top - 1) == 0 and lib.hd_fits(top, 5, top - 2 ** 26) == 1
    assert lib.hd_fits(top + 1, 5, 5) == 0 and lib.hd_fits(5, top + 1, 5) == 0 and lib.hd_fits(5, 5, top) == 0
    assert lib.hd_fits(0, 0, 1) == 1 and lib.hd_fits(2 ** 40, 1, 1) == 0
    # the sort's bits: the smallest b >= 1 with 2^b > ncells, so that the key ncells of a non-finite point is told apart
    for ncells, bits in ((1, 1), (2, 2), (3, 2), (4, 3), (255, 8), (256, 9), (2 ** 31 - 2, 31)):
        assert lib.hd_key_bits(ncells) == bits, ncells
