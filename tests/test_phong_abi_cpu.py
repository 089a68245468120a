"""CPU: what the four Phong entries refuse, and in which order (sizes, then pointers, then workspace).  Argument validation
is reachable without a GPU (tests/test_abi.py); every call here is refused or returns before it would launch, so a
pointer only has to be non-NULL."""
import ctypes

import pytest

from dss_amd import _lib

_buf = ctypes.create_string_buffer(64)
PTR = ctypes.addressof(_buf)            # never dereferenced: no call of this file gets as far as a launch
LEAD = ("world", "normals", "rgb", "first_idx", "num_pts", "N", "Pw", "shared", "ambient", "kd", "ks", "lvec", "L",
        "point_lights", "cam", "shininess")
ENTRIES = {   # name -> (argument names in the order of include/dss_hip.h without the stream, reducing entry)
    "dss_phong_forward": (LEAD + ("out",), False),
    "dss_phong_backward": (("grad_out",) + LEAD + ("grad_world", "grad_normals", "grad_rgb"), False),
    "dss_phong_backward_camera": (("grad_out",) + LEAD + ("grad_cam", "ws", "ws_bytes"), True),
    "dss_phong_backward_lights": (("grad_out",) + LEAD + ("grad_ambient", "grad_diffuse", "grad_specular", "grad_light_vec",
                                                          "ws", "ws_bytes"), True),
}
POINTS, REDUCING = [e for e, v in ENTRIES.items() if not v[1]], [e for e, v in ENTRIES.items() if v[1]]
SCALARS = {"N": 2, "Pw": 300, "shared": 0, "L": 2, "point_lights": 1, "shininess": 12.0, "ws_bytes": 1 << 30}
LIGHTS = ("kd", "ks", "lvec")


def call(entry, **over):
    """-> (return code, dss_last_error()) of `entry` with every pointer non-NULL and SCALARS, but for `over`"""
    vals = dict({k: PTR for k in ENTRIES[entry][0]}, **SCALARS)
    vals.update(over)
    rc = getattr(_lib.load(), entry)(*[vals[k] for k in ENTRIES[entry][0]], None)
    return rc, _lib.load().dss_last_error().decode()


def need_bytes(entry, N, Pw, L, shared=0):
    lib, P = _lib.load(), (N * Pw if shared else Pw)
    return lib.dss_camera_backward_workspace(N, P) if entry.endswith("camera") else lib.dss_phong_backward_lights_workspace(N, P, L)


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("bad", [{"N": 0}, {"N": -1}, {"Pw": -1}, {"L": -1}], ids=str)
def test_bad_sizes_are_refused_before_anything_else(entry, bad):
    sizes = dict({k: SCALARS[k] for k in ("N", "Pw", "L")}, **bad)
    text = "%s: bad sizes N=%d Pw=%d L=%d" % (entry, sizes["N"], sizes["Pw"], sizes["L"])
    assert call(entry, **bad) == (-1, text)
    assert call(entry, **dict({k: None for k in ENTRIES[entry][0] if k not in SCALARS}, **bad)) == (-1, text)


@pytest.mark.parametrize("entry", REDUCING)
def test_a_grid_dimension_beyond_65535_is_refused(entry):
    """cameras are gridDim.y of both reducing entries, lights gridDim.z of the lights entry alone; at 65535 the sizes pass
    and the call is refused later, at its NULL workspace"""
    short = "%s: workspace %d bytes < required %%d" % (entry, 1 << 30)
    assert call(entry, N=65536) == (-1, "%s: bad sizes N=65536 Pw=300 L=2" % entry)
    assert call(entry, N=65536, world=None, ws=None) == (-1, "%s: bad sizes N=65536 Pw=300 L=2" % entry)
    assert call(entry, N=65535, ws=None) == (-1, short % need_bytes(entry, 65535, 300, 2))
    assert call(entry, L=65535, ws=None) == (-1, short % need_bytes(entry, 2, 300, 65535))
    if entry == "dss_phong_backward_lights":
        assert call(entry, L=65536) == (-1, "%s: bad sizes N=2 Pw=300 L=65536" % entry)
    else:
        assert call(entry, L=65536, ws=None) == (-1, short % need_bytes(entry, 2, 300, 65536))


@pytest.mark.parametrize("entry", POINTS)
def test_the_points_entries_have_no_grid_limit(entry):
    """N = 65536, L = 65536 pass the size check of the points entries: the refusal is the later one, of the output"""
    last = "out" if entry == "dss_phong_forward" else "grad_out"
    rc, text = call(entry, N=65536, L=65536, **{last: None})
    assert rc == -1 and text == "%s: NULL %s" % (entry, "output" if last == "out" else "grad_out")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_required_pointer_null_in_turn(entry):
    names, reducing = ENTRIES[entry]
    required = ["world", "normals", "rgb", "first_idx", "num_pts", "ambient", "cam"] + list(LIGHTS)
    if reducing:
        required.append("grad_out")
    if entry == "dss_phong_backward_camera":
        required.append("grad_cam")
    for k in required:
        assert call(entry, **{k: None}) == (-1, "%s: NULL tensor pointer" % entry), k
    # the pointer check comes before the workspace's
    if reducing:
        assert call(entry, world=None, ws=None, ws_bytes=0) == (-1, "%s: NULL tensor pointer" % entry)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_light_tensors_are_needed_only_with_lights(entry):
    last = {"dss_phong_forward": "out", "dss_phong_backward": "grad_out"}.get(entry, "ws")
    rc, text = call(entry, L=0, kd=None, ks=None, lvec=None, **{last: None})   # refused later, at `last`
    assert rc == -1 and "NULL tensor pointer" not in text, text
    for k in LIGHTS:
        assert call(entry, L=1, **{k: None}) == (-1, "%s: NULL tensor pointer" % entry), k


def test_null_out_and_grad_out_of_the_points_entries():
    assert call("dss_phong_forward", out=None) == (-1, "dss_phong_forward: NULL output")
    assert call("dss_phong_backward", grad_out=None) == (-1, "dss_phong_backward: NULL grad_out")
    # ... after the tensor pointers
    assert call("dss_phong_forward", out=None, rgb=None) == (-1, "dss_phong_forward: NULL tensor pointer")
    assert call("dss_phong_backward", grad_out=None, rgb=None) == (-1, "dss_phong_backward: NULL tensor pointer")


@pytest.mark.parametrize("entry", POINTS)
def test_no_points_is_ok_with_every_pointer_null(entry):
    nulls = {k: None for k in ENTRIES[entry][0] if k not in SCALARS}
    assert call(entry, Pw=0, **nulls)[0] == 0
    assert call(entry, Pw=0, L=0, **nulls)[0] == 0
    assert call(entry, Pw=0, N=0, **nulls) == (-1, "%s: bad sizes N=0 Pw=0 L=2" % entry)


@pytest.mark.parametrize("entry", REDUCING)
def test_no_points_still_needs_the_ranges_the_centres_and_the_output(entry):
    """Pw = 0 on a reducing entry: stage 2 would launch to write zeros, so only the refusals are here"""
    inputs = {k: None for k in ("grad_out", "world", "normals", "rgb", "ambient") + LIGHTS}
    always = ["first_idx", "num_pts", "cam"] + (["grad_cam"] if entry.endswith("camera") else [])
    for k in always:
        assert call(entry, Pw=0, **dict(inputs, **{k: None})) == (-1, "%s: NULL tensor pointer" % entry), k
    need = need_bytes(entry, 2, 0, 2)
    assert call(entry, Pw=0, ws=None, **inputs) == (-1, "%s: workspace %d bytes < required %d" % (entry, 1 << 30, need))


@pytest.mark.parametrize("shared", [0, 1])
@pytest.mark.parametrize("entry", REDUCING)
def test_workspace_null_or_one_byte_short(entry, shared):
    need = need_bytes(entry, 2, 300, 2, shared)
    assert need > 0
    assert call(entry, shared=shared, ws=None, ws_bytes=need) == (-1, "%s: workspace %d bytes < required %d" % (entry, need, need))
    assert call(entry, shared=shared, ws_bytes=need - 1) == (-1, "%s: workspace %d bytes < required %d" % (entry, need - 1, need))
