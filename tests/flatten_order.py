"""The flatten order and the world transforms of a descriptor, restated in numpy for the tests that derive expected surface
data from the descriptor alone (test_gpu_surface.py, test_surface_oracle_cpu.py): models ascending; within a model its mesh
nodes in scene-graph (DFS pre-order) order, their primitives' triangles and spheres, then the model's quad lights, two
triangles each."""
import numpy as np

from rayca_amd import abi


def quat_mul(a, b):
    return np.array([a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0], -a[0] * b[2] + a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[1] - a[1] * b[0] + a[2] * b[3] + a[3] * b[2], -a[0] * b[0] - a[1] * b[1] - a[2] * b[2] + a[3] * b[3]])


def rotate(v, q):
    u, s = q[:3], q[3]
    return 2.0 * np.dot(u, v) * u + (s * s - np.dot(u, u)) * v + 2.0 * s * np.cross(u, v)


def conj(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def world_trs(desc):
    """float64 (translation, rotation, scale) per node, composed as Trs x Trs (trs.rs:211-221)"""
    out = []
    for n in desc._nodes[:desc.c.node_count]:
        t, q, s = (np.array(list(x), np.float64) for x in (n.trs.translation, n.trs.rotation, n.trs.scale))
        if n.parent >= 0:
            pt, pq, ps = out[n.parent]
            t, q, s = pt + rotate(ps * t, pq), quat_mul(pq, q), rotate(ps * rotate(s, q), conj(q))
        out.append((t, q, s))
    return out


def flat_table(desc):
    """per flattened primitive: node, descriptor primitive (-1: a quad light's triangle), triangle number, material, sphere?"""
    c = desc.c
    nodes = desc._nodes[:c.node_count]
    children = [[] for _ in nodes]
    tops = []
    for i, n in enumerate(nodes):
        (children[n.parent] if n.parent >= 0 else tops).append(i)
    order, stack = [], tops[::-1]
    while stack:
        n = stack.pop()
        order.append(n)
        stack.extend(children[n][::-1])
    mesh_nodes = [n for n in order if nodes[n].mesh != abi.NONE]
    quad_nodes = [n for n in order if nodes[n].light != abi.NONE and desc._lights[nodes[n].light].kind == abi.LIGHT_QUAD]
    rows = []
    for model in sorted({nodes[n].model for n in mesh_nodes + quad_nodes}):
        for n in mesh_nodes:
            if nodes[n].model != model:
                continue
            mesh = desc._meshes[nodes[n].mesh]
            for pi in range(mesh.first_primitive, mesh.first_primitive + mesh.primitive_count):
                p = desc._prims[pi]
                if p.geometry == abi.GEOMETRY_SPHERE:
                    rows.append((n, pi, 0, p.material, 1))
                else:
                    rows += [(n, pi, k, p.material, 0) for k in range(p.index_count // 3)]
        for n in quad_nodes:
            if nodes[n].model == model:
                rows += [(n, -1, k, desc._lights[nodes[n].light].material, 0) for k in range(2)]
    return np.array(rows, np.int64).reshape(-1, 5)
