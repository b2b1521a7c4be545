"""tests/gbuffer_model.py on analytic answers whose every intermediate is exact in float32 (the style of
tests/kat_analytic.py): the model that the GPU tests hold the G-buffer's normal and albedo planes to is
itself held to values worked out by hand, bit for bit (a -0.0 is not a 0.0)."""
import numpy as np

import gbuffer_model as gm

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, want, what):
    assert np.array_equal(bits(got), bits(want)), f"{what}: {np.asarray(got).tolist()} != {np.asarray(want).tolist()}"


def flipped(p, I, D):
    """Scene::GetNormal through the model's ray form: O = I - D, t = 1 (exact for the values used here)"""
    I, D = np.asarray(I, f32).reshape(-1, 3), np.asarray(D, f32).reshape(-1, 3)
    O = (I - D).astype(f32)
    assert np.array_equal(bits(gm.hit_point(O, D, np.ones(len(I), f32))), bits(I))
    return gm.normals([p], np.zeros(len(I), np.int32), O, D, np.ones(len(I), f32))


def test_hit_point_is_o_plus_t_times_d():
    O = f32([[1, 2, 3], [0.5, -0.25, 8]])
    D = f32([[0, 0, 1], [0.5, 0.5, -0.5]])
    t = f32([4, 2])
    same_bits(gm.hit_point(O, D, t), [[1, 2, 7], [1.5, 0.75, 7]], "I")


def test_sphere_normals_at_axis_points(rt):
    unit = rt.sphere((0, 0, 0), 1.0, 1)
    for axis in range(3):
        for s in (1.0, -1.0):
            I = np.zeros(3, f32)
            I[axis] = s
            same_bits(gm.prim_normal(unit, I), [I], f"unit sphere {I.tolist()}")
            same_bits(flipped(unit, I, -I), [I], "seen from outside: kept")             # dot(N, D) = -1
            same_bits(flipped(unit, I, I), [-I], "seen from inside: flipped")           # dot(N, D) = +1
    off = rt.sphere((2, -1, 4), 0.5, 1)                                                  # 1 / r = 2
    same_bits(gm.prim_normal(off, [2.5, -1, 4]), [[1, 0, 0]], "offset sphere +x")
    same_bits(gm.prim_normal(off, [2, -1.5, 4]), [[0, -1, 0]], "offset sphere -y")
    same_bits(gm.prim_normal(off, [2, -1, 3.5]), [[0, 0, -1]], "offset sphere -z")
    same_bits(gm.prim_normal(off, [2.25, -1.25, 4]), [[0.5, -0.5, 0]], "offset sphere, unnormalised as the reference leaves it")


def test_axis_planes_from_both_sides(rt):
    for axis in range(3):
        n = np.zeros(3, f32)
        n[axis] = 1
        p = rt.plane(tuple(float(x) for x in n), 1.0, 1)
        I = f32([0.25, 0.5, -0.75])
        same_bits(gm.prim_normal(p, I), [n], "plane normal = data[0]")
        same_bits(flipped(p, I, -n), [n], "from the front")
        same_bits(flipped(p, I, n), [-n], "from behind: every component negated, zeros to -0")
        assert np.signbit(flipped(p, I, n)).all()
        same_bits(flipped(p, I, np.roll(n, 1)), [n], "grazing (dot = 0): not flipped")


def test_axis_aligned_cube_six_faces(rt):
    for pos in ((0, 0, 0), (2, 0, -4)):
        c = rt.cube(pos, 2.0, 1)
        P = f32(pos)
        faces = [((1, 0.25, 0.5), (1, 0, 0)), ((-1, 0.25, 0.5), (-1, 0, 0)), ((0.25, 1, -0.5), (0, 1, 0)),
                 ((0.25, -1, -0.5), (0, -1, 0)), ((0.5, 0.25, 1), (0, 0, 1)), ((0.5, 0.25, -1), (0, 0, -1))]
        for local, n in faces:
            I = (f32(local) + P).astype(f32)
            same_bits(gm.prim_normal(c, I), [f32(n)], f"cube at {pos} face {n}")
            same_bits(flipped(c, I, f32(n)), [-f32(n)], f"cube at {pos} face {n} from inside")
    # an edge point is equally near two faces: the first of them in the reference's order keeps it
    same_bits(gm.prim_normal(rt.cube((0, 0, 0), 2.0, 1), [1, 1, 0]), [[1, 0, 0]], "edge +x/+y: x is tested first")
    same_bits(gm.prim_normal(rt.cube((0, 0, 0), 2.0, 1), [0, -1, 1]), [[0, -1, 0]], "edge -y/+z: y is tested first")


def test_cube_transform_matches_the_records(rt):
    """prim_transform's M for a rotated, offset cube equals the library's own matrix product"""
    T = rt.mat4_rotate(1, 0.5)
    c = rt.cube((1.5, 0, 2), 1.0, 1, T)
    M, Minv = gm.prim_transform(c)
    same_bits(M, rt.mat4_mul(T, rt.mat4_translate(1.5, 0, 2)), "Transform = T * Translate(pos)")
    back = gm.transform_position(Minv, gm.transform_position(M, f32([0.25, -0.5, 1])))
    assert np.abs(back - f32([0.25, -0.5, 1])).max() < 1e-5, back   # FastInvertedTransformNoScale undoes a rigid motion


def test_quad_and_triangle_normals(rt):
    q = rt.quad(1.0, 0)
    same_bits(gm.prim_normal(q, [0.25, 0, 0.25]), [[0, -1, 0]], "quad: TransformVector((0, -1, 0), identity)")
    same_bits(flipped(q, [0.25, 0, 0.25], [0, -1, 0]), [[-0.0, 1, -0.0]], "quad seen from above")
    t = rt.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), 1)                  # cross(C - A, B - A) = (0, 0, -1)
    same_bits(gm.prim_normal(t, [0.25, 0.25, 0]), [[0, 0, -1]], "triangle in z = 0")
    same_bits(flipped(t, [0.25, 0.25, 0], [0, 0, 1]), [[0, 0, -1]], "against +z: kept")
    same_bits(flipped(t, [0.25, 0.25, 0], [0, 0, -1]), [[-0.0, -0.0, 1]], "against -z: flipped")
    t2 = rt.triangle((0, 0, 0), (0, 0, 3), (4, 0, 0), 1)                # cross((4,0,0), (0,0,3)) = (0, -12, 0): 1/sqrt(144)
    same_bits(gm.prim_normal(t2, [1, 0, 1]), [[0, f32(-12) * (f32(1) / f32(12)), 0]], "triangle in y = 0")


def test_checkerboard_cells_around_negative_coordinates():
    c1, c2 = (1, 0.5, 0.25), (0, 0.125, 2)
    #            x      floor  even
    xs = [(-0.5, -1, False), (-1.0, -1, False), (-2.0, -2, True), (-1.5, -2, True), (0.0, 0, True), (-0.0, 0, True),
          (0.5, 0, True), (1.0, 1, False), (1.999, 1, False), (2.0, 2, True), (-3.0, -3, False), (-2.5, -3, False)]
    for x, fx, ex in xs:
        assert int(np.floor(f32(x))) == fx
        for z, fz, ez in xs:
            got = gm.checkerboard_color([[x, 7.5, z]], c1, c2)
            same_bits(got, [c1 if ex == ez else c2], f"cell ({x}, {z})")


def test_texture_texel_borders_4x2():
    #  texel (x, y) holds red = 16 * (x + 4 * y), green = 255 - that, blue = 0: every texel distinct
    tex = np.array([[((16 * (x + 4 * y)) << 16) | ((255 - 16 * (x + 4 * y)) << 8) for x in range(4)] for y in range(2)],
                   np.uint32)
    k = f32(1.0) / f32(255.0)

    def want(x, y):
        r = 16 * (x + 4 * y)
        return [f32(r) * k, f32(255 - r) * k, f32(0)]

    below = np.nextafter(f32(0.25), f32(0))
    cases = [(0.0, 0.0, 0, 0), (0.25, 0.0, 1, 0), (below, 0.0, 0, 0), (0.5, 0.5, 2, 1), (0.75, np.nextafter(f32(0.5), f32(0)), 3, 0),
             (1.0, 1.0, 0, 0),                      # 4 & 3, 2 & 1: the wrap
             (1.25, 1.5, 1, 1), (-0.25, 0.0, 3, 0),  # uint(-1.0) = 0xffffffff & 3
             (-0.5, -0.5, 2, 1), (0.999, 0.999, 3, 1)]
    for u, v, x, y in cases:
        same_bits(gm.texture_color(tex, f32([u]), f32([v])), [want(x, y)], f"u {u} v {v}")
    same_bits(gm.texture_color(tex, f32([0.0]), f32([0.0]))[0, 2:], [0.0], "a zero byte is 0.0 exactly")
