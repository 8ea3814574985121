"""Triangle meshes for Scene.MakeMesh: a Wavefront OBJ reader and two generators, so that demos, tests and measurements need no file.

Every function returns (vertices float32 (n, 3), faces uint32 (m, 3)) but the ones that say otherwise.  load_obj ignores a file's normals; load_obj_normals
reads them, vertex_normals makes area-weighted ones for a mesh without, icosphere_normals gives the sphere's own (smooth shading).  load_obj_uvs
reads a file's texture coordinates, uv_sphere makes a sphere with the ones an image-textured sphere has; without any a triangle takes them from
its own plane.  load_obj_materials reads a file's `usemtl` groups and `mtllib` names, load_mtl the `Kd` and `map_Kd` of an MTL file (the scene's
texture table).
"""
import numpy as np


def _obj_index(token, n_vertices, where):
    """the vertex index of an `i`, `i/j`, `i/j/k` or `i//k` token: 1-based, or negative = counted back from the vertices read so far"""
    try:
        i = int(token.split("/")[0])
    except ValueError:
        raise ValueError(f"{where}: bad face index {token!r}") from None
    k = i - 1 if i > 0 else n_vertices + i
    if i == 0 or not 0 <= k < n_vertices:
        raise ValueError(f"{where}: face index {token!r} out of range ({n_vertices} vertices so far)")
    return k


def load_obj(path):
    """`v x y z` and `f a b c ...` lines of a Wavefront OBJ file; a polygon of more than three corners is cut into a fan around its first corner;
    every other line (vn, vt, g, o, s, usemtl, mtllib, comments) is ignored."""
    vertices, faces = [], []
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        for lineno, line in enumerate(f, 1):
            parts = line.split("#", 1)[0].split()
            if not parts:
                continue
            where = f"{path}:{lineno}"
            if parts[0] == "v":
                if len(parts) < 4:
                    raise ValueError(f"{where}: a vertex needs three coordinates")
                vertices.append([float(parts[1]), float(parts[2]), float(parts[3])])
            elif parts[0] == "f":
                if len(parts) < 4:
                    raise ValueError(f"{where}: a face needs at least three corners")
                corners = [_obj_index(t, len(vertices), where) for t in parts[1:]]
                for k in range(1, len(corners) - 1):
                    faces.append([corners[0], corners[k], corners[k + 1]])
    return np.array(vertices, np.float32).reshape(-1, 3), np.array(faces, np.uint32).reshape(-1, 3)


def _obj_third(token, n_normals, where):
    """the normal index of an `i/j/k` or `i//k` token (1-based, negative = counted back from the normals read so far), or None for a token without one"""
    parts = token.split("/")
    if len(parts) < 3 or parts[2] == "":
        return None
    try:
        i = int(parts[2])
    except ValueError:
        raise ValueError(f"{where}: bad normal index {token!r}") from None
    k = i - 1 if i > 0 else n_normals + i
    if i == 0 or not 0 <= k < n_normals:
        raise ValueError(f"{where}: normal index {token!r} out of range ({n_normals} normals so far)")
    return k


def load_obj_normals(path):
    """load_obj that keeps the normals: (vertices, faces, normals float32 (k, 3) | None, normal_faces uint32 (m, 3) | None) from the `v`, `vn` and `f` lines;
    the third index of an `i/j/k` or `i//k` corner names its normal (negative indices and fans as for vertices).  A file without `vn` lines, or one face
    corner without a normal index, gives None, None: the mesh has no complete set of normals (vertex_normals makes one)."""
    vertices, faces, normals, normal_faces = [], [], [], []
    complete = True
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        for lineno, line in enumerate(f, 1):
            parts = line.split("#", 1)[0].split()
            if not parts:
                continue
            where = f"{path}:{lineno}"
            if parts[0] == "v":
                if len(parts) < 4:
                    raise ValueError(f"{where}: a vertex needs three coordinates")
                vertices.append([float(parts[1]), float(parts[2]), float(parts[3])])
            elif parts[0] == "vn":
                if len(parts) < 4:
                    raise ValueError(f"{where}: a normal needs three coordinates")
                normals.append([float(parts[1]), float(parts[2]), float(parts[3])])
            elif parts[0] == "f":
                if len(parts) < 4:
                    raise ValueError(f"{where}: a face needs at least three corners")
                corners = [_obj_index(t, len(vertices), where) for t in parts[1:]]
                thirds = [_obj_third(t, len(normals), where) for t in parts[1:]]
                if any(k is None for k in thirds):
                    complete = False
                for k in range(1, len(corners) - 1):
                    faces.append([corners[0], corners[k], corners[k + 1]])
                    if complete:
                        normal_faces.append([thirds[0], thirds[k], thirds[k + 1]])
    v, fa = np.array(vertices, np.float32).reshape(-1, 3), np.array(faces, np.uint32).reshape(-1, 3)
    if not normals or not complete:
        return v, fa, None, None
    return v, fa, np.array(normals, np.float32).reshape(-1, 3), np.array(normal_faces, np.uint32).reshape(-1, 3)


def _obj_second(token, n_uvs, where):
    """the texture-coordinate index of an `i/j` or `i/j/k` token (1-based, negative = counted back from the `vt` lines read so far), or None for a token without one"""
    parts = token.split("/")
    if len(parts) < 2 or parts[1] == "":
        return None
    try:
        i = int(parts[1])
    except ValueError:
        raise ValueError(f"{where}: bad texture coordinate index {token!r}") from None
    k = i - 1 if i > 0 else n_uvs + i
    if i == 0 or not 0 <= k < n_uvs:
        raise ValueError(f"{where}: texture coordinate index {token!r} out of range ({n_uvs} texture coordinates so far)")
    return k


def load_obj_uvs(path):
    """load_obj that keeps the texture coordinates: (vertices, faces, uvs float32 (k, 2) | None, uv_faces uint32 (m, 3) | None) from the `v`, `vt` and `f` lines;
    the second index of an `i/j` or `i/j/k` corner names its `vt` (negative indices and fans as for vertices; a third coordinate of a `vt` line is dropped).
    A file without `vt` lines, or one face corner without a second index, gives None, None: the mesh has no complete set of texture coordinates."""
    vertices, faces, uvs, uv_faces = [], [], [], []
    complete = True
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        for lineno, line in enumerate(f, 1):
            parts = line.split("#", 1)[0].split()
            if not parts:
                continue
            where = f"{path}:{lineno}"
            if parts[0] == "v":
                if len(parts) < 4:
                    raise ValueError(f"{where}: a vertex needs three coordinates")
                vertices.append([float(parts[1]), float(parts[2]), float(parts[3])])
            elif parts[0] == "vt":
                if len(parts) < 3:
                    raise ValueError(f"{where}: a texture coordinate needs two values")
                uvs.append([float(parts[1]), float(parts[2])])
            elif parts[0] == "f":
                if len(parts) < 4:
                    raise ValueError(f"{where}: a face needs at least three corners")
                corners = [_obj_index(t, len(vertices), where) for t in parts[1:]]
                seconds = [_obj_second(t, len(uvs), where) for t in parts[1:]]
                if any(k is None for k in seconds):
                    complete = False
                for k in range(1, len(corners) - 1):
                    faces.append([corners[0], corners[k], corners[k + 1]])
                    if complete:
                        uv_faces.append([seconds[0], seconds[k], seconds[k + 1]])
    v, fa = np.array(vertices, np.float32).reshape(-1, 3), np.array(faces, np.uint32).reshape(-1, 3)
    if not uvs or not complete:
        return v, fa, None, None
    return v, fa, np.array(uvs, np.float32).reshape(-1, 2), np.array(uv_faces, np.uint32).reshape(-1, 3)


def load_obj_materials(path):
    """The material groups of a Wavefront OBJ file: (names, libraries) — per triangle of load_obj's faces (a polygon's fan shares one) the name its `usemtl`
    line gave it, None before the first; and the file names of the `mtllib` lines in order.  Nothing else is read."""
    names, libraries, current = [], [], None
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        for lineno, line in enumerate(f, 1):
            parts = line.split("#", 1)[0].split()
            if not parts:
                continue
            if parts[0] == "usemtl":
                current = parts[1] if len(parts) > 1 else None
            elif parts[0] == "mtllib":
                libraries.extend(parts[1:])
            elif parts[0] == "f":
                if len(parts) < 4:
                    raise ValueError(f"{path}:{lineno}: a face needs at least three corners")
                names.extend([current] * (len(parts) - 3))
    return names, libraries


def load_mtl(path):
    """`newmtl`, `Kd` and `map_Kd` of a Wavefront MTL file: {name: {"Kd": (r, g, b) | None, "map_Kd": path | None}} in the file's order; the image's name is
    resolved beside the file, options in front of it (-s, -o, ...) are skipped.  `norm`, `map_Bump`, `map_bump` and `bump` name the material's normal map
    (the file is taken as a tangent-space normal map, OpenGL convention, green = +v): "normal_map": path | None and "normal_strength": the `-bm X`
    in front of the name, 1.0 without one; the last such line of a material counts.  The PBR extension's `Pr`, `map_Pr` and `Pm` become
    "roughness": float | None, "roughness_map": path | None and "metallic": float | None.  The keywords glass is told by add keys of their own, each
    present only when the file has the keyword: `Ni` as "ior" (> 0), `d` and `Tr` as "dissolve" in [0, 1] (Tr = 1 - d), `illum` as "illum" (an integer).  `Tf r g b` (or `Tf r`), the
    transmission filter (the tint of solid glass), likewise: "transmission_filter": (r, g, b), each finite and in [0, 1]; its `spectral` and `xyz`
    forms are not read.  `map_d` (the opacity image of an alpha cutout) likewise: "cutout_map": path, resolved beside the file, options in front of
    the name skipped.  Nothing else of MTL is read."""
    import os
    out, current = {}, None
    beside = lambda name: os.path.join(os.path.dirname(os.path.abspath(path)), *name.replace("\\", "/").split("/"))
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        for lineno, line in enumerate(f, 1):
            parts = line.split("#", 1)[0].split()
            if not parts:
                continue
            where = f"{path}:{lineno}"
            if parts[0] == "newmtl":
                if len(parts) < 2:
                    raise ValueError(f"{where}: newmtl needs a name")
                current = out.setdefault(parts[1], {"Kd": None, "map_Kd": None, "normal_map": None, "normal_strength": 1.0, "roughness": None, "roughness_map": None,
                                                    "metallic": None})
            elif parts[0] in ("norm", "map_Bump", "map_bump", "bump"):
                if current is None:
                    raise ValueError(f"{where}: {parts[0]} before any newmtl")
                if len(parts) < 2:
                    raise ValueError(f"{where}: {parts[0]} needs a file name")
                strength = 1.0
                if "-bm" in parts[1:-1]:
                    at = parts.index("-bm", 1)
                    if at + 1 >= len(parts) - 1:
                        raise ValueError(f"{where}: -bm needs a value in front of the file name")
                    strength = float(parts[at + 1])
                    if not (np.isfinite(strength) and strength >= 0.0):
                        raise ValueError(f"{where}: -bm must be finite and >= 0")
                current["normal_map"], current["normal_strength"] = beside(parts[-1]), strength
            elif parts[0] in ("Pr", "Pm", "map_Pr"):
                if current is None:
                    raise ValueError(f"{where}: {parts[0]} before any newmtl")
                if len(parts) < 2:
                    raise ValueError(f"{where}: {parts[0]} needs a {'file name' if parts[0] == 'map_Pr' else 'value'}")
                if parts[0] == "map_Pr":
                    current["roughness_map"] = beside(parts[-1])
                else:
                    value = float(parts[1])
                    if not (np.isfinite(value) and 0.0 <= value <= 1.0):
                        raise ValueError(f"{where}: {parts[0]} must be finite and in [0, 1]")
                    current["roughness" if parts[0] == "Pr" else "metallic"] = value
            elif parts[0] in ("Ni", "d", "Tr", "illum"):
                if current is None:
                    raise ValueError(f"{where}: {parts[0]} before any newmtl")
                if len(parts) < 2:
                    raise ValueError(f"{where}: {parts[0]} needs a value")
                if parts[0] == "illum":
                    try:
                        current["illum"] = int(parts[1])
                    except ValueError:
                        raise ValueError(f"{where}: illum must be an integer") from None
                else:
                    value = float(parts[-1])   # (`d -halo x`: the option is skipped)
                    if parts[0] == "Ni":
                        if not (np.isfinite(value) and value > 0.0):
                            raise ValueError(f"{where}: Ni must be finite and above 0")
                        current["ior"] = value
                    else:
                        if not (np.isfinite(value) and 0.0 <= value <= 1.0):
                            raise ValueError(f"{where}: {parts[0]} must be finite and in [0, 1]")
                        current["dissolve"] = value if parts[0] == "d" else 1.0 - value
            elif parts[0] == "map_d":   # §34: the opacity image of a cutout material; options in front of the name (-imfchan, -s, ...) are skipped
                if current is None:
                    raise ValueError(f"{where}: map_d before any newmtl")
                if len(parts) < 2:
                    raise ValueError(f"{where}: map_d needs a file name")
                current["cutout_map"] = beside(parts[-1])
            elif parts[0] == "Tf":
                if current is None:
                    raise ValueError(f"{where}: Tf before any newmtl")
                if len(parts) >= 2 and parts[1] in ("spectral", "xyz"):
                    continue
                if len(parts) not in (2, 4):
                    raise ValueError(f"{where}: Tf needs one value or three")
                rgb = tuple(float(x) for x in (parts[1:4] if len(parts) == 4 else parts[1:2] * 3))
                if not all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in rgb):
                    raise ValueError(f"{where}: Tf must be finite and in [0, 1]")
                current["transmission_filter"] = rgb
            elif parts[0] in ("Kd", "map_Kd"):
                if current is None:
                    raise ValueError(f"{where}: {parts[0]} before any newmtl")
                if parts[0] == "Kd":
                    if len(parts) < 4:
                        raise ValueError(f"{where}: Kd needs three values")
                    current["Kd"] = (float(parts[1]), float(parts[2]), float(parts[3]))
                else:
                    if len(parts) < 2:
                        raise ValueError(f"{where}: map_Kd needs a file name")
                    current["map_Kd"] = os.path.join(os.path.dirname(os.path.abspath(path)), *parts[-1].replace("\\", "/").split("/"))
    return out


def uv_sphere(n_lon, n_lat):
    """a latitude-longitude unit sphere: (vertices (n, 3), faces (m, 3), normals (n, 3), uvs (n, 2)), n = (n_lat + 1) (n_lon + 1), m = 2 n_lon (n_lat - 1).
    Vertex (j, i) has u = i / n_lon, v = j / n_lat and stands where an image-textured sphere has that (u, v) (sphere::get_sphere_uv: theta = pi v from -y,
    phi = 2 pi u): (-cos(phi) sin(theta), -cos(theta), sin(phi) sin(theta)).  The seam column i = n_lon repeats i = 0 with u = 1, and each pole is one vertex per
    column, so every coordinate lies in [0, 1] and no face spans the seam.  The normals are the positions; faces are counter-clockwise seen from outside."""
    if n_lon < 3 or n_lat < 2:
        raise ValueError("uv_sphere: at least 3 columns and 2 rows")
    u = np.arange(n_lon + 1, dtype=np.float64) / n_lon
    v = np.arange(n_lat + 1, dtype=np.float64) / n_lat
    theta, phi = np.pi * v[:, None], 2.0 * np.pi * u[None, :]
    pos = np.stack([-np.cos(phi) * np.sin(theta), -np.cos(theta) * np.ones_like(phi), np.sin(phi) * np.sin(theta)], axis=-1).reshape(-1, 3)
    uv = np.stack(np.broadcast_arrays(u[None, :], v[:, None]), axis=-1).reshape(-1, 2)
    at = lambda j, i: j * (n_lon + 1) + i
    faces = []
    for j in range(n_lat):
        for i in range(n_lon):
            if j > 0:               # not at the south pole, where (j, i) and (j, i + 1) coincide
                faces.append([at(j, i), at(j + 1, i + 1), at(j, i + 1)])
            if j < n_lat - 1:       # not at the north pole
                faces.append([at(j, i), at(j + 1, i), at(j + 1, i + 1)])
    f = np.array(faces, np.int64)
    outward = (np.cross(pos[f[:, 1]] - pos[f[:, 0]], pos[f[:, 2]] - pos[f[:, 0]]) * pos[f].mean(axis=1)).sum(axis=1)
    f[outward < 0] = f[outward < 0][:, [0, 2, 1]]
    nrm = pos / np.linalg.norm(pos, axis=1)[:, None]
    return pos.astype(np.float32), f.astype(np.uint32), nrm.astype(np.float32), uv.astype(np.float32)


def vertex_normals(vertices, faces):
    """area-weighted vertex normals of an indexed mesh, float32 (n, 3): per vertex the sum of cross(b - a, c - a) over its faces (twice the face's area
    along its normal), normalised in float64; a vertex no face uses, or whose sum vanishes, gets (0, 0, 1)"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, f[:, k], fn)
    ln = np.linalg.norm(acc, axis=1)
    out = np.where((ln > 0)[:, None], acc / np.where(ln > 0, ln, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
    return out.astype(np.float32)


def icosphere_normals(level):
    """the vertex normals of icosphere(level): its unit positions, float32 (n, 3)"""
    return icosphere(level)[0].copy()


def tetrahedron():
    """a regular tetrahedron inscribed in the unit sphere, faces counter-clockwise seen from outside"""
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) / np.sqrt(3.0)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.uint32)
    return v.astype(np.float32), f


def icosphere(level):
    """an icosahedron subdivided `level` times (every triangle into four, new vertices pushed out to the unit sphere): 20 * 4**level faces,
    10 * 4**level + 2 vertices, closed — every edge belongs to exactly two faces"""
    if not 0 <= int(level) <= 7:
        raise ValueError("icosphere: level must be 0..7")
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    v = [list(np.array(p, np.float64) / np.linalg.norm(p)) for p in v]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(int(level)):
        mid = {}

        def midpoint(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in mid:
                m = (np.array(v[a]) + np.array(v[b])) * 0.5
                v.append(list(m / np.linalg.norm(m)))
                mid[key] = len(v) - 1
            return mid[key]

        nf = []
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.array(v, np.float32), np.array(f, np.uint32)


def _welded(vertices, faces):
    """the faces over welded vertices — those closer than 1e-6 of the mesh's extent are one, so the seam and the poles of uv_sphere, or an OBJ that repeats a
    position per texture coordinate, are closed — without the faces that welding leaves degenerate"""
    v, f = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    if len(v) == 0 or len(f) == 0:
        return f
    extent = float((v.max(axis=0) - v.min(axis=0)).max())
    cell = np.round((v - v.min(axis=0)) / (1e-6 * extent)).astype(np.int64) if extent > 0.0 else np.zeros(v.shape, np.int64)
    f = np.unique(cell, axis=0, return_inverse=True)[1].reshape(-1)[f]
    return f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]


def _edge_census(vertices, faces):
    """{(a, b): how many faces run the edge from a to b} over the directed edges of the faces, vertices welded"""
    f = _welded(vertices, faces)
    census = {}
    for a, b in np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist():
        census[(a, b)] = census.get((a, b), 0) + 1
    return census


def signed_volume(vertices, faces):
    """the volume the faces enclose by the divergence theorem, in double: positive when they are wound counter-clockwise seen from outside"""
    v, f = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def consistently_closed(vertices, faces):
    """True when every edge is shared by exactly two faces that run it in opposite directions: a closed surface, consistently wound one way or the other"""
    census = _edge_census(vertices, faces)
    return len(census) > 0 and all(n == 1 and census.get((b, a), 0) == 1 for (a, b), n in census.items())


def closed_outward(vertices, faces):
    """True when the mesh is closed and consistently wound (consistently_closed) and its signed volume is positive: what the facing rule of solid glass
     trusts — the stored normal of every face points out of the solid.  Vertices that coincide are one vertex: a seam of duplicated vertices is closed."""
    return consistently_closed(vertices, faces) and signed_volume(vertices, faces) > 0.0


def orient_outward(vertices, faces):
    """The faces wound outward: as they are when closed_outward holds, every face flipped when the mesh is consistently wound and closed but inside out.
    Raises ValueError for an open or inconsistently wound mesh, and for one that encloses no volume: such a mesh has no inside, and guessing one is not this
    function's business."""
    f = np.asarray(faces).reshape(-1, 3)
    if not consistently_closed(vertices, f):
        raise ValueError("orient_outward: the mesh is open or its faces are not consistently wound (every edge must be shared by exactly two faces, in opposite directions)")
    volume = signed_volume(vertices, f)
    if volume == 0.0 or not np.isfinite(volume):
        raise ValueError("orient_outward: the mesh encloses no volume")
    return f.copy() if volume > 0.0 else np.ascontiguousarray(f[:, ::-1])


def from_spec(spec):
    """`icosphere:LEVEL`, `tetrahedron`, or the path of an OBJ file (tools/render.py --mesh)"""
    if spec.startswith("icosphere:"):
        return icosphere(int(spec.split(":", 1)[1]))
    if spec == "tetrahedron":
        return tetrahedron()
    return load_obj(spec)
