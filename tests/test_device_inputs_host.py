"""The package's device-input front end (octree-tracer_amd/_device.py) on the CPU device, and the signature
tables of _lib.py against the headers.  No GPU needed: the converter and the list front end are plain tensor code."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

CPU = types.SimpleNamespace(torch_device=torch.device("cpu"))  # what the front end asks of a Gpu


def u32(pkg, a, **kw):
    t = pkg._device.device_u32(a, CPU.torch_device, **kw)
    assert t.dtype == torch.int32 and t.is_contiguous()
    return t.numpy().astype(np.int64).tolist()


def test_clamp_keeps_out_of_range_values_out_of_range(pkg):
    assert u32(pkg, np.array([[-5, 3, 2**40]], dtype=np.int64), clamp=True) == [[-1, 3, 2147483647]]
    assert u32(pkg, np.array([[1, 2, 2**31 + 5]], dtype=np.uint32), clamp=True) == [[1, 2, 2147483647]]
    assert u32(pkg, np.array([[3, 0, 300]], dtype=np.int16), clamp=True) == [[3, 0, 300]]
    assert u32(pkg, np.array([[0, 17, 255]], dtype=np.uint8), clamp=True) == [[0, 17, 255]]


def test_mask_is_applied_to_every_integer_dtype(pkg):
    assert u32(pkg, np.array([0x1FFFFFF, -1], dtype=np.int64), mask=0xFFFFFF) == [0xFFFFFF, 0xFFFFFF]
    assert u32(pkg, torch.tensor([0x1FFFFFF, -1], dtype=torch.int32), mask=0xFFFFFF) == [0xFFFFFF, 0xFFFFFF]


def test_cells_stay_non_zero_iff_they_were(pkg):
    assert u32(pkg, np.array([0, 5, 1 << 24, 1 << 40], dtype=np.int64), cells=True) == [0, 0x1000005, 0x1000000, 0x1000000]


@pytest.mark.parametrize("bad", [np.zeros(3, dtype=np.float32), np.zeros(3, dtype=bool), np.zeros(3, dtype=np.complex64),
                                 torch.zeros(3, dtype=torch.float32)])
def test_non_integer_input_is_refused(pkg, bad):
    with pytest.raises(TypeError, match=r"^integer input expected, got "):
        pkg._device.device_u32(bad, CPU.torch_device, clamp=True)
    with pytest.raises(TypeError, match=r"^triangles: integer input expected, got "):
        pkg._device.device_u32(bad, CPU.torch_device, clamp=True, what="triangles")


def test_voxel_list_checks_and_pointers(pkg):
    V = pkg._device.voxel_list
    with pytest.raises(ValueError, match=r"^coords must be \(N, 3\), got \(4, 2\)$"):
        V(CPU, np.zeros((4, 2), dtype=np.int64))
    with pytest.raises(ValueError, match=r"^3 colours for 4 voxels$"):
        V(CPU, np.zeros((4, 3), dtype=np.int64), np.arange(3))
    with pytest.raises(ValueError, match=r"^triangles must be \(T, 3\), got \(4, 2\)$"):
        V(CPU, np.zeros((4, 2), dtype=np.int64), noun="triangles", what="triangles", rows="T")
    with pytest.raises(ValueError, match=r"^3 colours for 4 triangles$"):
        V(CPU, np.zeros((4, 3), dtype=np.int64), np.arange(3), noun="triangles", what="triangles", rows="T")
    with pytest.raises(TypeError, match=r"^colours: integer input expected"):
        V(CPU, np.zeros((4, 3), dtype=np.int64), np.zeros(4, dtype=np.float32), noun="triangles", what="triangles", rows="T")
    xyz, col, n, xyz_ptr, col_ptr = V(CPU, np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert n == 0 and xyz_ptr is None and col_ptr is None and tuple(xyz.shape) == (0, 3)
    xyz, col, n, xyz_ptr, col_ptr = V(CPU, np.array([[1, 2, 3], [-4, 5, 2**35]]), None)
    assert n == 2 and col is None and col_ptr is None and xyz_ptr == xyz.data_ptr()
    assert xyz.tolist() == [[1, 2, 3], [-1, 5, 2147483647]]
    xyz, col, n, xyz_ptr, col_ptr = V(CPU, [[1, 2, 3], [4, 5, 6]], np.array([[0x1234567], [-1]]))
    assert n == 2 and col.tolist() == [0x234567, 0xFFFFFF] and col_ptr == col.data_ptr()


def test_an_empty_float_list_is_refused_like_any_other(pkg):
    """np.zeros((0, 3)) without a dtype is float64: empty or not, it is refused, as it always was (the empty list of
    test_voxel_list_checks_and_pointers therefore names an integer dtype)"""
    with pytest.raises(TypeError):
        pkg._device.voxel_list(CPU, np.zeros((0, 3)))


# declarations the simple parse below cannot count (none today); name them here rather than drop the check
UNPARSED = ()


def test_signature_tables_have_the_headers_parameter_counts(pkg):
    """every entry of _lib's two tables has as many argument types as its declaration in include/ has parameters"""
    counts = {}
    for h, table in (("svo_hip.h", pkg._lib.DEVICE_SIGNATURES), ("svo_host.h", pkg._lib.HOST_SIGNATURES)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        for name, params in re.findall(r"\b(svo_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
            params = params.strip()
            counts[name] = 0 if params in ("", "void") else params.count(",") + 1
        for name, (res, args) in table.items():
            if name in UNPARSED:
                continue
            assert name in counts, f"{name}: in the table of {h} but its declaration there was not found"
            assert len(args) == counts[name], f"{name}: {len(args)} argument types, {h} declares {counts[name]} parameters"
    assert len(counts) >= 50 and set(pkg._lib.DEVICE_SIGNATURES).isdisjoint(pkg._lib.HOST_SIGNATURES)
