"""The built scene of the tile-occlusion tests (tests/test_tile_occlusion_host.py, tests/test_gpu_tile_occlusion.py):
a radius-1 sphere in front of five small ones and a ground sphere, seen on a 64×48 frame by a camera whose view the
front sphere nearly fills — most tiles lie inside its silhouette and lose the ground and the small spheres behind it —
plus the placements that must not fool the culling (csrc/rt_tile_entry.h tile_occlusion), each as extra spheres or
another camera."""
import numpy as np

from cudaraytracer_amd import abi, scenes

WIDTH, HEIGHT = 64, 48
EYE = (0.0, 2.0, 5.0)
FRONT_C, FRONT_R = (0.0, 1.0, 1.0), 1.0
GROUND = ((0.0, -100.0, 0.0), 100.0)
SMALL = [((0.0, 1.0, -1.5), 0.25), ((-0.8, 0.6, -1.5), 0.25), ((0.8, 0.6, -1.5), 0.25), ((-0.6, 1.5, -1.5), 0.25),
         ((0.6, 1.5, -1.5), 0.25)]
GROUND_INDEX, FRONT_INDEX, FIRST_EXTRA = 0, 1, 2 + len(SMALL)


def _toward_eye(distance):
    """The point at `distance` from the front sphere's centre on the segment to the eye."""
    v = np.array(EYE) - np.array(FRONT_C)
    return tuple(float(x) for x in np.array(FRONT_C) + distance * v / np.linalg.norm(v))


# name -> extra spheres (hittables FIRST_EXTRA …)
PLACEMENTS = {
    "plain": [],
    # a small sphere poking through the front one inside the beam: nearer than the front sphere for some rays
    "poke": [(_toward_eye(0.95), 0.15)],
    # tangent to the front sphere from outside, on the eye's side and on the far side
    "tangent": [(_toward_eye(1.2), 0.2), (_toward_eye(-1.2), 0.2)],
    # concentric and smaller: hidden for every ray that hits the front sphere
    "concentric": [(FRONT_C, 0.5)],
    # the eye inside a sphere: every ray leaves it before anything else
    "eye_inside": [(EYE, 0.8)],
}


def scene(placement="plain") -> scenes.Scene:
    spheres = [GROUND, (FRONT_C, FRONT_R)] + SMALL + PLACEMENTS[placement]
    h = (abi.HittableDesc * len(spheres))()
    m = (abi.MaterialDesc * 3)()
    for k, (t, col) in enumerate([(abi.RT_LAMBERTIAN, (0.5, 0.5, 0.5)), (abi.RT_METAL, (0.8, 0.6, 0.2)),
                                  (abi.RT_DIELECTRIC, (1.0, 1.0, 1.0))]):
        m[k].type, m[k].fuzz, m[k].ir = t, 0.1, 1.5
        m[k].albedo.type, m[k].albedo.image = abi.RT_CONSTANT, -1
        m[k].albedo.color[:] = list(col)
    for i, (c, r) in enumerate(spheres):
        h[i].type, h[i].is_active, h[i].radius, h[i].material = abi.RT_SPHERE, 1, float(r), i % 3
        h[i].center[:] = [float(x) for x in c]
    return scenes.Scene(h, m, [])


NEAR_EYE = _toward_eye(1.2)  # from here the rays start inside the front sphere, 0.35 ahead of the eye


def inputs(eye=EYE, fov=26.0):
    """The camera: from `eye` toward the front sphere's centre.  At fov 26 the front sphere's silhouette crosses the
    frame's outer tiles and holds the inner ones."""
    fwd = scenes.normalized(tuple(c - e for c, e in zip(FRONT_C, eye)))
    return scenes.camera_inputs(eye, fwd, fov)
