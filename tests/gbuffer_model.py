"""A float32 numpy restatement of what the G-buffer's normal and albedo planes hold at a hit, in the
reference's operation order (a helper, not a test): numpy rounds every float32 operation on its own and
never fuses a multiply with an add, so each result's bits are defined.

  I = O + t * D                            Ray::IntersectionPoint (Ray.h:21)
  Primitive::GetNormal, all five kinds     Primitive.h:284-314 (the cube's nearest face, TransformVector)
  the flip against the ray                 Scene::GetNormal, template/scene.h:495
  Checkerboard::GetColor                   Checkerboard.h:28-37
  TextureMaterial::GetColor                TextureMaterial.h:32-39

No transcendental is restated here: the tests take sky and light colours from the oracle's Trace.
Primitives are the library's records (rt.sphere / plane / triangle / cube / quad; cubes and quads carry
their mat4 in .T), materials its rt.material records; only their fields are read."""
import numpy as np

f32 = np.float32
FLT_EPSILON = f32(1.192092896e-07)
SPHERE, PLANE, CUBE, QUAD, TRIANGLE = 0, 1, 2, 3, 4
CHECKERBOARD, TEXTURE = 3, 6


def _a(x):
    return np.asarray(x, f32)


def dot(a, b):
    """precomp.h:805: (x*x' + y*y') + z*z'"""
    a, b = _a(a), _a(b)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    a, b = _a(a), _a(b)
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(f32)


def normalize(v):
    """precomp.h:827, 473: v * (1 / sqrt(dot(v, v)))"""
    v = _a(v)
    inv = f32(1) / np.sqrt(dot(v, v)).astype(f32)
    return (v * inv[..., None]).astype(f32)


def _rows(M, a, w):
    """make_float3(float4(a, w) * M), template.cpp:825-839: ((m0*x + m1*y) + m2*z) + m3*w per row"""
    M, a = _a(M).reshape(-1)[:12].reshape(3, 4), _a(a)
    return np.stack([((M[r, 0] * a[..., 0] + M[r, 1] * a[..., 1]) + M[r, 2] * a[..., 2]) + M[r, 3] * f32(w)
                     for r in range(3)], -1).astype(f32)


def transform_position(M, a):
    return _rows(M, a, 1.0)


def transform_vector(M, a):
    return _rows(M, a, 0.0)


IDENTITY = np.eye(4, dtype=f32).reshape(16)


def mat4_mul(a, b):
    """precomp.h:1007-1085: row i of a times column j of b, summed left to right"""
    a, b = _a(a).reshape(16), _a(b).reshape(16)
    r = np.zeros(16, f32)
    for i in range(0, 16, 4):
        for j in range(4):
            r[i + j] = ((a[i] * b[j] + a[i + 1] * b[j + 4]) + a[i + 2] * b[j + 8]) + a[i + 3] * b[j + 12]
    return r


def fast_inverse(c):
    """mat4::FastInvertedTransformNoScale, precomp.h:1061-1085"""
    c = _a(c).reshape(16)
    r = IDENTITY.copy()
    r[0], r[1], r[2] = c[0], c[4], c[8]
    r[4], r[5], r[6] = c[1], c[5], c[9]
    r[8], r[9], r[10] = c[2], c[6], c[10]
    r[3] = -((c[3] * r[0] + c[7] * r[1]) + c[11] * r[2])
    r[7] = -((c[3] * r[4] + c[7] * r[5]) + c[11] * r[6])
    r[11] = -((c[3] * r[8] + c[7] * r[9]) + c[11] * r[10])
    return r


def prim_transform(p):
    """Primitive::Transform / InvertedTransform (Primitive.h:28-29, 39-41, 690-737): Translate(centre)
    for a sphere, T * Translate(pos) (|pos| > FLT_EPSILON) or T for a cube, T for a quad, else identity."""
    v = _a(list(p.v))
    T = IDENTITY.copy() if getattr(p, "T", None) is None else _a(p.T).reshape(16)
    M = IDENTITY.copy()
    if p.type == SPHERE:
        M[3], M[7], M[11] = v[0], v[1], v[2]
    elif p.type == CUBE:
        if np.sqrt(dot(v[:3], v[:3])).astype(f32) > FLT_EPSILON:
            Tr = IDENTITY.copy()
            Tr[3], Tr[7], Tr[11] = v[0], v[1], v[2]
            M = mat4_mul(T, Tr)
        else:
            M = T
    elif p.type == QUAD:
        M = T
    return M, fast_inverse(M)


def hit_point(O, D, t):
    """I = O + t * D"""
    return (_a(O) + _a(t)[..., None] * _a(D)).astype(f32)


def prim_normal(p, I):
    """Primitive::GetNormal(I), Primitive.h:284-314, for the points I [n, 3] on primitive p (not flipped)"""
    I = _a(I).reshape(-1, 3)
    v = _a(list(p.v))
    n = len(I)
    if p.type == SPHERE:                                  # (I - centre) * data[0].z, data[0].z = 1 / r
        M, _ = prim_transform(p)
        centre = transform_position(M, np.zeros(3, f32))
        return ((I - centre) * (f32(1) / v[3])).astype(f32)
    if p.type == PLANE:                                   # data[0]
        return np.broadcast_to(v[:3], (n, 3)).astype(f32)
    if p.type == CUBE:
        M, Minv = prim_transform(p)
        o = transform_position(Minv, I)
        d0, d1 = f32(-0.5) * v[3:6], f32(0.5) * v[3:6]   # data[0], data[1] (Primitive.h:724-725)
        N = np.tile(_a([-1, 0, 0]), (n, 1))
        e = [np.abs(o[:, 0] - d0[0]), np.abs(o[:, 0] - d1[0]), np.abs(o[:, 1] - d0[1]), np.abs(o[:, 1] - d1[1]),
             np.abs(o[:, 2] - d0[2]), np.abs(o[:, 2] - d1[2])]
        mind = e[0].copy()
        for k, face in ((1, None), (2, (0, -1, 0)), (3, (0, 1, 0)), (4, (0, 0, -1)), (5, (0, 0, 1))):
            m = e[k] < mind
            mind = np.where(m, e[k], mind)
            if face is None:
                N[m, 0] = 1                              # "N.x = 1": the other components stay
            else:
                N[m] = _a(face)
        return transform_vector(M, N)
    if p.type == QUAD:
        M, _ = prim_transform(p)
        return np.broadcast_to(transform_vector(M, _a([0, -1, 0])), (n, 3)).astype(f32)
    base = normalize(cross(v[6:9] - v[0:3], v[3:6] - v[0:3]))   # TRIANGLE: C - A before B - A
    return np.broadcast_to(transform_vector(IDENTITY, base), (n, 3)).astype(f32)


def normals(prims, obj, O, D, t):
    """Scene::GetNormal(obj, I, D) per ray (obj >= 0 everywhere): Primitive::GetNormal at I = O + t*D,
    negated where dot(N, D) > 0 (template/scene.h:495)."""
    obj = np.asarray(obj)
    I = hit_point(O, D, t)
    N = np.zeros((len(obj), 3), f32)
    for k in np.unique(obj):
        m = obj == k
        N[m] = prim_normal(prims[int(k)], I[m])
    flip = dot(N, D) > 0
    N[flip] = -N[flip]
    return N


def checkerboard_color(I, color1, color2):
    """Checkerboard::GetColor: abs(((int) floor(I.x)) % 2) == 0 against the same of I.z"""
    I = _a(I).reshape(-1, 3)
    ix, iz = np.floor(I[:, 0]).astype(np.int64), np.floor(I[:, 2]).astype(np.int64)
    even_x, even_z = np.abs(np.fmod(ix, 2)) == 0, np.abs(np.fmod(iz, 2)) == 0
    return np.where((even_x == even_z)[:, None], _a(color1), _a(color2)).astype(f32)


def _to_uint(x):
    """float -> uint as the reference's x86-64 build converts: (uint32)(int64) trunc(x)"""
    return (np.trunc(_a(x).astype(np.float64)).astype(np.int64) & 0xffffffff).astype(np.int64)


def texture_color(tex, u, v):
    """TextureMaterial::GetColor: texel (uint(w * u) & (w - 1), uint(h * v) & (h - 1)), its three bytes
    as floats times 1 / 255 (`correction`)."""
    tex = np.asarray(tex, np.uint32)
    h, w = tex.shape
    ui, vi = _to_uint(f32(w) * _a(u)), _to_uint(f32(h) * _a(v))
    p = tex.reshape(-1)[(ui & (w - 1)) + (vi & (h - 1)) * w].astype(np.int64)
    rgb = np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], -1).astype(f32)
    return (rgb * (f32(1.0) / f32(255.0))).astype(f32)


def albedo(mat, textures, I, u, v):
    """The material's GetColor at the hit for the kinds that depend on it; every other kind's colour is
    its record's (None here: the caller compares with the material table)."""
    if mat.kind == CHECKERBOARD:
        return checkerboard_color(I, list(mat.color), list(mat.color2))
    if mat.kind == TEXTURE:
        return texture_color(textures[mat.texture], u, v)
    return None
