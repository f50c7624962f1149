"""RT_RADIANCE_DIRECT_LIGHT in rt_adaptive_samples and rt_temporal_gradient: the argument checks (CPU: no device call is
reached, every check precedes the first one and the reading of the scene).

Both calls accept the flag, alone and with the fill-order bit, and then get as far as "NULL scene"; with the flag
max_depth above 4096 is rejected by name, without it it is not; an empty list and an empty frame are RT_OK with the flag
and no device; the Python wrappers carry the new keyword arguments.  The other flag bits stay rejected: that is
test_adaptive_host.py's and test_gradient_host.py's, unchanged."""
from __future__ import annotations

import ctypes as C
import inspect

from cudaraytracer_amd import abi
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer

from test_adaptive_host import _samples_args
from test_direct_light_host import DIRECT
from test_gradient_host import GRADIENT_BUFFERS, H, W, _gradient_args
from test_radiance_host import _rejected

LTR = abi.RT_FLAG_RIUS_LEFT_TO_RIGHT
CALLS = (("rt_adaptive_samples", _samples_args), ("rt_temporal_gradient", _gradient_args))


def _call(who: str, a, scene=None) -> int:
    return getattr(lib(), who)(scene, C.byref(a), None)


def test_the_flag_is_the_header_s():
    assert DIRECT == abi.RT_RADIANCE_DIRECT_LIGHT == 1 << 8 and DIRECT & LTR == 0
    assert lib().rt_abi_version() == abi.ABI_VERSION == 14  # (no structure changed)


def test_both_calls_accept_the_flag():
    for who, make in CALLS:
        for flags in (DIRECT, DIRECT | LTR):
            a, keep = make()
            a.flags = flags
            _rejected(_call(who, a), who, "NULL scene")
        # ... and no other bit rides along with it
        for extra in (1, 2, 4, 16, abi.RT_FLAG_RNG_PHILOX, 1 << 9, 1 << 31):
            a, keep = make()
            a.flags = DIRECT | extra
            _rejected(_call(who, a), who, "flags")


def test_depth_limit_with_the_flag():
    bogus = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the arguments are checked first
    for who, make in CALLS:
        for flags in (DIRECT, DIRECT | LTR):
            for depth in (4097, 0xffffffff):
                a, keep = make()
                a.flags, a.max_depth = flags, depth
                _rejected(_call(who, a, bogus), who, "max_depth")
            a, keep = make()
            a.flags, a.max_depth = flags, 4096
            _rejected(_call(who, a), who, "NULL scene")
        for flags in (0, LTR):  # without the flag the depth is free
            a, keep = make()
            a.flags, a.max_depth = flags, 4097
            _rejected(_call(who, a), who, "NULL scene")


def test_nothing_to_do_is_accepted_without_a_device():
    for flags in (DIRECT, DIRECT | LTR):
        a, keep = _samples_args(0)
        a.flags = flags
        assert _call("rt_adaptive_samples", a) == 0
        a.pixels = None
        a.width = a.height = 0
        assert _call("rt_adaptive_samples", a) == 0
        a.max_depth = 4097  # ... but the arguments are still checked
        _rejected(_call("rt_adaptive_samples", a), "rt_adaptive_samples", "max_depth")
        for w, h in ((0, H), (W, 0), (0, 0)):
            a, keep = _gradient_args(w, h)
            a.flags = flags
            assert _call("rt_temporal_gradient", a) == 0
            for name in GRADIENT_BUFFERS:
                setattr(a, name, None)
            assert _call("rt_temporal_gradient", a) == 0
            a.max_depth = 4097
            _rejected(_call("rt_temporal_gradient", a), "rt_temporal_gradient", "max_depth")


def test_python_keywords():
    for fn in (DeviceScene.adaptive_samples, DeviceScene.temporal_gradient):
        p = inspect.signature(fn).parameters
        assert "direct_light" in p and p["direct_light"].default is False, fn
    p = inspect.signature(Renderer.adaptive).parameters
    assert p["direct_light"].default is None
    p = inspect.signature(Renderer.render_direct).parameters
    assert list(p)[1:] == ["scene", "inputs", "spp", "depth", "direct_light", "left_to_right"]
    assert (p["spp"].default, p["depth"].default, p["direct_light"].default, p["left_to_right"].default) == (1, 8, True, False)
