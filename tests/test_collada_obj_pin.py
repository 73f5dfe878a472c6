"""The Collada path pinned to data the reference itself holds.

The reference ships its startup scene twice: x64/Release/data/collada/cubes2.DAE (what
RayTracer.cpp:862 loads through ColladaLoader, ColladaLoader.cpp:13-593 + Mesh.cpp:10-78)
and x64/Release/data/models/cubes2.obj (the same 13 objects exported by 3ds Max, read by
the reference's loadObj, RayTracer.cpp:1008-1100).  The DAE is in inches (<unit
meter="0.0254"/>), the OBJ in centimetres about another origin, so OBJ = 2.54 * DAE + t.
This test loads both with the product loaders (rt_mesh_load_dae, rt_mesh_load_obj) and
with the Collada restatement oracle/dae_oracle.py, and checks per object, per triangle:

  * vertex positions: every transformed DAE vertex lies on an OBJ vertex (to the OBJ's
    printed 4 decimals plus float32 rounding at 2,300 cm);
  * triangles and winding: every DAE triangle is an OBJ triangle with the same cyclic
    vertex order (a mirrored transform or swapped winding fails);
  * normals: every corner's transformed DAE normal equals the OBJ's normal of that corner;
  * materials: every triangle carries the effect its <polygons material=...> names, by
    position in <library_effects> (parsed here independently of both loaders).

Two of the 13 objects (ChamferBox005/006) are the only ones with rotations about all three
axes.  The reference composes node rotations in a fixed order that maps rotateZ's angle to
a Y rotation and rotateY's to a Z rotation (ColladaLoader.cpp:499-537, `switch (i % 3)`
over {jointOrientX/Y/Z, rotateX, rotateZ, rotateY}), so its boxes come out oriented
differently from 3ds Max's export.  Those two are checked for that (they must NOT sit on
the OBJ's vertices: a loader that "fixed" the order would no longer be the reference's)
and for shape (same centroid distances up to the unit scale: a rigid motion of the OBJ's
box)."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import rtamd
from conftest import reference_data

DATA = reference_data()   # tests/golden/reference_data, unpacked
DAE = os.path.join(DATA, "collada", "cubes2.DAE")
OBJ = os.path.join(DATA, "models", "cubes2.obj")
INCH = 2.54
POS_TOL = 0.01    # cm: OBJ prints 4 decimals; float32 at |x| ~ 2300 cm is 2.4e-4; t from printed values
NRM_TOL = 2e-3    # OBJ prints unit normals with 4 decimals
THREE_AXIS = {"ChamferBox005", "ChamferBox006"}


def _local(tag):
    return tag.rsplit("}", 1)[-1]


def _dae_objects():
    """Per node (file order): name, geometry id, triangle count, material named by its polygons,
    and the rotate sids it has; plus the effect names in library order.  Parsed here, not by
    either loader."""
    root = ET.parse(DAE).getroot()
    lib = {_local(c.tag): c for c in root}
    effects = [e.get("name") for e in lib["library_effects"] if _local(e.tag) == "effect"]
    geos = {}
    for g in lib["library_geometries"]:
        polys = [p for p in g.iter() if _local(p.tag) == "polygons"][0]
        geos[g.get("id")] = (int(polys.get("count")), polys.get("material"))
    nodes = []
    vs = [c for c in lib["library_visual_scenes"] if _local(c.tag) == "visual_scene"][0]
    for nd in vs:
        if _local(nd.tag) != "node":
            continue
        inst = [c for c in nd if _local(c.tag) == "instance_geometry"][0]
        rots = {c.get("sid") for c in nd if _local(c.tag) == "rotate"}
        gid = inst.get("url")[1:]
        nodes.append((nd.get("id"), gid, geos[gid][0], geos[gid][1], rots))
    return effects, nodes, list(geos), [geos[g][0] for g in geos]


def _obj_groups():
    """Vertex and normal counts of each `# object` section of the OBJ, in file order."""
    groups = []
    for line in open(OBJ):
        if line.startswith("# object "):
            groups.append([line.split()[2], 0, 0])
        elif line.startswith("v "):
            groups[-1][1] += 1
        elif line.startswith("vn "):
            groups[-1][2] += 1
    return groups


@pytest.fixture(scope="module")
def meshes():
    from oracle import dae_oracle
    return rtamd.Mesh.load_dae(DAE).arrays(), dae_oracle.load_dae(DAE), rtamd.Mesh.load_obj(OBJ).arrays()


def test_dae_and_obj_describe_the_same_objects(meshes):
    _, nodes, geo_order, _ = _dae_objects()
    groups = _obj_groups()
    assert [g[0] for g in groups] == [n[0] for n in nodes if n[0] != "Sky001"][:len(groups)]
    d, _, o = meshes
    assert d["indices"].size == o["indices"].size == 3 * 23392


@pytest.mark.parametrize("which", ["product", "oracle"])
def test_collada_path_matches_the_reference_obj(meshes, which):
    from scipy.spatial import cKDTree
    d = meshes[0] if which == "product" else meshes[1]
    o = meshes[2]
    effects, nodes, geo_order, geo_tris = _dae_objects()
    groups = _obj_groups()

    # the DAE's triangles come geometry by geometry, in library order (Mesh.cpp:10-78); a node
    # instances one geometry and carries its transform
    tri0 = np.cumsum([0] + geo_tris)
    dv = d["vertices"][:, :3].astype(np.float64)
    dn = d["normals"][:, :3].astype(np.float64)
    di = d["indices"].reshape(-1, 3)
    dni = d["normals_indices"].reshape(-1, 3)
    ov = o["vertices"][:, :3].astype(np.float64)
    on = o["normals"][:, :3].astype(np.float64)
    oi = o["indices"].reshape(-1, 3)
    oni = o["normals_indices"].reshape(-1, 3)

    # OBJ = 2.54 * DAE + t, t from the ground plane (Plane001: the first object in both files)
    name0, gid0 = nodes[0][0], nodes[0][1]
    assert name0 == "Plane001" == groups[0][0]
    g0 = geo_order.index(gid0)
    pv = dv[np.unique(di[tri0[g0]:tri0[g0 + 1]])]
    qv = ov[:groups[0][1]]
    t = (qv.min(0) + qv.max(0)) / 2 - INCH * (pv.min(0) + pv.max(0)) / 2
    tree = cKDTree(ov)
    otri = {}
    for k, tri in enumerate(oi):
        for r in range(3):   # cyclic rotations keep the winding
            otri[tuple(np.roll(tri, -r))] = (k, r)

    checked = 0
    v_off = np.cumsum([0] + [g[1] for g in groups])
    for name, gid, ntri, material, rots in nodes:
        if name == "Sky001":
            continue
        g = geo_order.index(gid)
        sl = slice(tri0[g], tri0[g + 1])
        assert tri0[g + 1] - tri0[g] == ntri
        # materials: the effect the geometry's <polygons material=...> names, by library position
        assert np.all(d["tri_to_material"][sl] == effects.index(material)), name
        mapped = INCH * dv[np.unique(di[sl])] + t
        dist, _ = tree.query(mapped)
        if name in THREE_AXIS:
            # the reference's fixed rotation order (module docstring): off the OBJ's vertices ...
            assert dist.max() > 0.5, f"{name}: matches 3ds Max's orientation, not the reference loader's"
            # ... but the same rigid box: centroid distances agree
            gi = [i for i, gg in enumerate(groups) if gg[0] == name][0]
            box = ov[v_off[gi]:v_off[gi + 1]]
            r_dae = np.sort(np.linalg.norm(mapped - mapped.mean(0), axis=1))
            r_obj = np.sort(np.linalg.norm(box - box.mean(0), axis=1))
            assert r_dae.shape == r_obj.shape and np.max(np.abs(r_dae - r_obj)) < POS_TOL, name
            continue
        assert dist.max() < POS_TOL, f"{name}: a vertex is {dist.max():.4f} cm off the OBJ"
        # per triangle: the OBJ triangle on the same three vertices, same cyclic order
        _, near = tree.query(INCH * dv + t)
        for k in range(tri0[g], tri0[g + 1]):
            key = tuple(near[di[k]])
            assert key in otri, f"{name}: triangle {k} is not an OBJ triangle with the same winding"
            ok, r = otri[key]
            for c in range(3):
                n_d = dn[dni[k, c]]
                n_o = on[oni[ok, (c + r) % 3]]
                assert np.max(np.abs(n_d - n_o)) < NRM_TOL, f"{name}: normal of triangle {k} corner {c}"
            checked += 1
    assert checked == 23392 - 2 * 2760
