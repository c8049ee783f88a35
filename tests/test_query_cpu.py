"""The device-buffer ray queries without a GPU: the Python validation (raised before the library is reached) and the entry points' answers
on a host-only scene and on a null scene."""
import ctypes as C

import numpy as np
import pytest

from conftest import asset

import raytracerwin_amd as R

RTW_ERR_INVALID, RTW_ERR_NO_DEVICE = -1, -2


@pytest.fixture(scope="module")
def host_scene():
    s = R.RayTracerScene(None)
    s.AddShape(R.RMeshShape.Create(asset("TorusKnot.obj")), R.SurfaceMaterial_Diffuse())
    s.commit()
    yield s
    s.close()


def test_python_validation_comes_before_the_library(host_scene):
    torch = pytest.importorskip("torch")
    s = host_scene
    with pytest.raises(ValueError, match="CPU"):
        s.trace_closest(torch.zeros((4, 7), dtype=torch.float32))
    with pytest.raises(ValueError, match="CPU"):
        s.trace_occluded(torch.zeros((4, 7), dtype=torch.float32))
    with pytest.raises(ValueError, match="float32"):
        s.trace_closest(torch.zeros((4, 7), dtype=torch.float64))
    with pytest.raises(ValueError, match="7"):
        s.trace_closest(torch.zeros((4, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        s.trace_closest(torch.zeros((7, 4), dtype=torch.float32).t())
    with pytest.raises(ValueError, match="torch tensor"):
        s.trace_closest(np.zeros((4, 7), np.float32))
    with pytest.raises(ValueError, match="float32"):
        s.trace_occluded(np.zeros((4, 7), np.float64))
    with pytest.raises(ValueError, match="7"):
        s.trace_occluded(np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        s.trace_occluded(np.zeros((7, 4), np.float32).T)


def test_host_only_and_null_scenes(host_scene):
    L = R.library()
    rays = np.zeros((2, 7), np.float32)
    rays[:, 5] = 1
    rays[:, 6] = 10
    out = np.zeros(64, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = host_scene.h
    assert L.rtw_trace_closest_device(h, p(rays), C.c_int64(2), None, p(out), None) == RTW_ERR_NO_DEVICE
    assert L.rtw_trace_occluded_device(h, p(rays), C.c_int64(2), p(out)) == RTW_ERR_NO_DEVICE
    assert L.rtw_trace_occluded(h, p(rays), C.c_int64(2), p(out)) == RTW_ERR_NO_DEVICE
    assert L.rtw_trace_closest_device(None, p(rays), C.c_int64(2), None, p(out), None) == RTW_ERR_INVALID
    assert L.rtw_trace_occluded_device(None, p(rays), C.c_int64(2), p(out)) == RTW_ERR_INVALID
    assert L.rtw_trace_occluded(None, p(rays), C.c_int64(2), p(out)) == RTW_ERR_INVALID
    assert L.rtw_trace_closest_device(h, p(rays), C.c_int64(2), None, None, None) == RTW_ERR_INVALID
    assert not out.any()
    with pytest.raises(R.RtwError):
        host_scene.trace_occluded(rays)
