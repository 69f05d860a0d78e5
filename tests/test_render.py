"""softrod_render without a GPU: the three entry points are declared, exported and bound and the ABI stays 17; the
ctypes camera mirrors the C struct and _capi.camera_default its C twin for every env kind; every refusal of
softrod_camera_check; and self-checks of the NumPy reference the GPU test compares with (tests/render_ref.py)."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from gym_softrobot_amd import _capi

try:
    from tests import render_ref as ref
except ImportError:                                  # imported with tests/ itself on the path
    import render_ref as ref

ROOT = Path(__file__).resolve().parents[1]
EINVAL = -1
NAMES = ("softrod_camera_default", "softrod_camera_check", "softrod_render")

BUILDERS = [
    ("softpendulum", _capi.softpendulum_config),
    ("softpendulum3d", _capi.softpendulum3d_config),
    ("arm_single", _capi.arm_single_config),
    ("octo_flat", _capi.octo_flat_config),
    ("soft_arm", _capi.soft_arm_config),
    ("arm_push", _capi.arm_push_config),
    ("arm_pull_weight", _capi.arm_pull_weight_config),
    ("crawl", lambda n: _capi.muscle_octopus_config(_capi.ENV_CRAWL, n)),
    ("arm_two", lambda n: _capi.muscle_octopus_config(_capi.ENV_ARM_TWO, n)),
    ("reach", lambda n: _capi.muscle_octopus_config(_capi.ENV_REACH, n)),
]


def test_names_are_declared_exported_and_the_abi_stays_17(hip_lib):
    header = (ROOT / "include" / "softrod.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\(", code), name
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
    assert "typedef struct softrod_camera {" in code
    assert "#define SOFTROD_ABI_VERSION 17" in header
    assert _capi.ABI_VERSION == 17 and hip_lib.softrod_abi_version() == 17
    assert hip_lib.softrod_render.argtypes == [C.c_void_p, C.POINTER(_capi.SoftrodCamera), C.c_void_p, C.c_void_p, C.c_void_p]


def test_palette_mirrors_the_header():
    header = (ROOT / "include" / "softrod.h").read_text()
    words = re.search(r"#define SOFTROD_RENDER_PALETTE\s*\\\s*\{([^}]*)\}", header).group(1)
    pal = [int(w.strip().rstrip("u"), 16) for w in words.split(",")]
    assert [((p >> 16) & 255, (p >> 8) & 255, p & 255) for p in pal] == [tuple(c) for c in _capi.RENDER_PALETTE]
    assert len(pal) == 10
    bg = int(re.search(r"#define SOFTROD_RENDER_BACKGROUND (0x[0-9A-Fa-f]+)u", header).group(1), 16)
    assert ((bg >> 16) & 255, (bg >> 8) & 255, bg & 255) == tuple(_capi.RENDER_BACKGROUND)
    # the bodies can be told apart by colour family at every shade the model produces (ambient >= 0: down to black
    # they cannot, so the comparison asks for it on lit frames): neighbouring palette rays are at least 5 degrees apart
    P = np.array(_capi.RENDER_PALETTE, float)
    U = P / np.linalg.norm(P, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip(U @ U.T, -1, 1))) + 360 * np.eye(10)
    assert ang.min() > 5.0


@pytest.mark.parametrize("name,builder", BUILDERS, ids=[b[0] for b in BUILDERS])
def test_camera_default_mirrors_its_c_twin(hip_lib, name, builder):
    cfg = builder(5)
    c = _capi.SoftrodCamera()
    c.width = 7                                                    # stale contents must not survive
    assert hip_lib.softrod_camera_default(C.byref(cfg), C.byref(c)) == 0
    py = _capi.camera_default(cfg)
    assert c.struct_size == C.sizeof(_capi.SoftrodCamera) == 136
    assert bytes(c) == bytes(py), name
    assert (c.width, c.height) == (84, 84)
    assert hip_lib.softrod_camera_check(C.byref(c)) == 0
    assert c.follow == (1 if cfg.features & _capi.FEAT_OCTO_HEAD else 0)
    n = np.cross(np.array(c.right), np.array(c.up))
    if name in ("softpendulum3d", "soft_arm"):
        assert n[2] > 0 and abs(n[2]) < 1                          # oblique, from above
    else:
        assert n.tolist() == [0.0, 0.0, 1.0]                       # along -z: x right, y up
    assert hip_lib.softrod_camera_default(None, C.byref(c)) == EINVAL
    assert hip_lib.softrod_camera_default(C.byref(cfg), None) == EINVAL


def _cam():
    return _capi.camera_default(_capi.softpendulum_config(2))


def _set(field, value):
    def edit(cam):
        if isinstance(field, tuple):
            getattr(cam, field[0])[field[1]] = value
        else:
            setattr(cam, field, value)
    return edit


REFUSALS = [
    ("struct_size", _set("struct_size", 8)),
    ("width 0", _set("width", 0)),
    ("width 1025", _set("width", 1025)),
    ("height 0", _set("height", 0)),
    ("height 1025", _set("height", 1025)),
    ("nan center", _set(("center", 1), float("nan"))),
    ("inf half_width", _set("half_width", float("inf"))),
    ("nan light", _set(("light", 0), float("nan"))),
    ("nan ambient", _set("ambient", float("nan"))),
    ("inf target_radius", _set("target_radius", float("inf"))),
    ("half_width 0", _set("half_width", 0.0)),
    ("half_width negative", _set("half_width", -1.0)),
    ("right not unit", _set(("right", 0), 1.0 + 3e-6)),
    ("up not unit", _set(("up", 1), 1.0 - 3e-6)),
    ("axes not orthogonal", _set(("up", 0), 3e-6)),
    ("light not unit", _set(("light", 2), 0.64 + 5e-6)),
    ("ambient negative", _set("ambient", -0.01)),
    ("ambient above 1", _set("ambient", 1.01)),
    ("target_radius negative", _set("target_radius", -1e-3)),
    ("follow 2", _set("follow", 2)),
]


@pytest.mark.parametrize("what,edit", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_camera_check_refuses(hip_lib, what, edit):
    cam = _cam()
    assert hip_lib.softrod_camera_check(C.byref(cam)) == 0
    edit(cam)
    assert hip_lib.softrod_camera_check(C.byref(cam)) == EINVAL, what
    assert b"render:" in hip_lib.softrod_last_error(None), what


def test_camera_check_accepts_what_is_inside_the_tolerances(hip_lib):
    cam = _cam()
    cam.right[0] = 1.0 + 5e-7
    cam.up[0] = 5e-7
    cam.width, cam.height = 1024, 1
    cam.ambient = 1.0
    cam.target_radius = 0.0
    assert hip_lib.softrod_camera_check(C.byref(cam)) == 0
    assert hip_lib.softrod_camera_check(None) == EINVAL and b"render:" in hip_lib.softrod_last_error(None)


def test_render_refuses_null_arguments_before_any_device_is_needed(hip_lib):
    cam = _cam()
    assert hip_lib.softrod_render(None, C.byref(cam), None, None, None) == EINVAL
    assert hip_lib.softrod_last_error(None) == b"render: null handle"


# ---- the reference's own checks ----

def _scene(A, B, r, body):
    A, B = np.asarray(A, float)[None], np.asarray(B, float)[None]
    return ref.Prims(A, B, np.asarray(r, float), np.asarray(body, int), np.zeros((1, 3)))


def _camera(w, h, hw):
    cam = _cam()
    cam.width, cam.height, cam.half_width = w, h, hw
    return cam


def test_reference_sphere_area_and_centre_colour():
    cam = _camera(81, 61, 1.0)                        # odd sizes: a pixel centre sits on the sphere's centre
    r = 0.3
    f = ref.render(_scene([[0, 0, 0]], [[0, 0, 0]], [r], [3]), cam)
    pixel = 2.0 / 81
    covered = int((f.body[0] == 3).sum())
    # the silhouette's perimeter in pixels bounds the miscount of a pixel-centre rule
    assert abs(covered - math.pi * r * r / pixel ** 2) <= 2 * math.pi * r / pixel
    assert (f.depth[0] > -np.inf).sum() == covered
    lz, amb = cam.light[2], cam.ambient
    want = np.floor(255 * np.array(_capi.RENDER_PALETTE[3]) / 255.0 * (amb + (1 - amb) * lz) + 0.5)
    assert f.rgb[0, 30, 40].tolist() == want.tolist()
    assert f.depth[0, 30, 40] == pytest.approx(r, abs=1e-15)           # the pole, towards the viewer
    assert (f.rgb[0, 0, 0] == ref.BACKGROUND).all() and f.depth[0, 0, 0] == -np.inf and f.body[0, 0, 0] == -1


def test_reference_crossing_capsules_resolve_to_the_nearer():
    cam = _camera(64, 64, 1.0)
    lo = ([-0.8, 0, 0.0], [0.8, 0, 0.0])             # along x at depth 0
    hi = ([0, -0.8, 0.5], [0, 0.8, 0.5])             # along y, nearer the viewer (n = +z)
    f = ref.render(_scene([lo[0], hi[0]], [lo[1], hi[1]], [0.1, 0.1], [0, 1]), cam)
    centre = f.body[0, 30:34, 30:34]
    assert (centre == 1).all()
    assert (f.body[0, 32, 5] == 0) and (f.body[0, 5, 32] == 1)
    # listed the other way round the picture is the same: depth, not order, decides
    g = ref.render(_scene([hi[0], lo[0]], [hi[1], lo[1]], [0.1, 0.1], [1, 0]), cam)
    assert np.array_equal(f.rgb, g.rgb) and np.array_equal(f.depth, g.depth)
    # at EQUAL depth the lowest index wins
    e = ref.render(_scene([lo[0], [0, -0.8, 0.0]], [lo[1], [0, 0.8, 0.0]], [0.1, 0.1], [0, 1]), cam)
    for i in range(30, 34):                          # on the diagonals |u| = |v|: both surfaces at the same z
        assert e.body[0, i, i] == 0 and e.body[0, i, 63 - i] == 0
        assert e.undecided[0, i, i] and e.undecided[0, i, 63 - i]      # two bodies within the band of each other
    assert e.body[0, 33, 31] == 1 and not e.undecided[0, 33, 31]       # nearer the y capsule's axis: its surface is higher
    assert e.body[0, 31, 33] == 0 and not e.undecided[0, 31, 33]


def test_reference_mirrors_with_the_right_axis():
    rng = np.random.default_rng(0)
    A, B = rng.uniform(-0.7, 0.7, (6, 3)), rng.uniform(-0.7, 0.7, (6, 3))
    sc = _scene(A, B, np.full(6, 0.06), np.arange(6))
    cam = _camera(48, 32, 1.0)
    f = ref.render(sc, cam)
    cam.right[0] = -1.0                               # n = a x b flips too: the viewer goes to the other side
    g = ref.render(sc, cam)
    assert np.array_equal(g.body[0] >= 0, (f.body[0] >= 0)[:, ::-1])       # the silhouette mirrors
    cam.light[0] = -cam.light[0]
    sc2 = _scene(A * [1, 1, -1], B * [1, 1, -1], np.full(6, 0.06), np.arange(6))   # ... and with z reflected, so does the frame
    g2 = ref.render(sc2, cam)
    assert np.array_equal(g2.rgb[0], f.rgb[0][:, ::-1])
    hit = g2.body[0] >= 0
    assert np.array_equal(hit, (f.body[0] >= 0)[:, ::-1])
    assert np.abs(g2.depth[0][hit] - f.depth[0][:, ::-1][hit]).max() < 1e-12


def test_reference_non_finite_primitive_covers_nothing_and_follow_centres():
    cam = _camera(32, 32, 1.0)
    A = [[0, 0, 0], [np.nan, 0, 0], [0.2, 0.2, 0]]
    B = [[0.5, 0, 0], [0.5, 0.5, 0], [0.2, np.inf, 0]]
    f = ref.render(_scene(A, B, [0.1, 0.1, 0.1], [0, 1, 2]), cam)
    g = ref.render(_scene(A[:1], B[:1], [0.1], [0]), cam)
    assert np.array_equal(f.rgb, g.rgb) and set(np.unique(f.body)) == {-1, 0}
    far = np.array([100.0, -50.0, 0.0])
    sc = ref.Prims(np.asarray(A[:1], float)[None] + far, np.asarray(B[:1], float)[None] + far, np.array([0.1]), np.array([0]),
                   far[None])
    cam.follow = 1
    h = ref.render(sc, cam)
    assert np.array_equal(h.body, g.body) and np.abs(h.depth[h.body >= 0] - g.depth[g.body >= 0]).max() < 1e-12


def test_reference_primitive_order_from_state_arrays():
    """primitives(): rods in arm order at their stride, then head, then target."""
    cfg = _capi.octo_flat_config(2)
    ne, na, seg = int(cfg.n_elem), int(cfg.n_arm), 16
    rng = np.random.default_rng(1)
    st = {"position": rng.normal(size=(3, 2, 128)), "head": rng.normal(size=(20, 2)), "control": np.zeros((4, 2)),
          "arm_stride": seg}
    p = ref.primitives(cfg, st)
    assert p.A.shape == (2, na * ne + 2, 3) and p.body.tolist() == sum(([a] * ne for a in range(na)), []) + [8, 9]
    assert np.array_equal(p.A[1, 3 * ne + 2], st["position"][:, 1, 3 * seg + 2])
    assert np.array_equal(p.B[1, 3 * ne + 2], st["position"][:, 1, 3 * seg + 3])
    assert np.array_equal(p.A[0, na * ne], st["head"][0:3, 0]) and np.array_equal(p.anchor, st["head"][0:3].T)
    assert p.A[1, -1].tolist() == [st["head"][18, 1], st["head"][19, 1], 0.0]
    assert (p.r[:na * ne] == cfg.base_radius).all() and p.r[na * ne] == cfg.head_radius
