"""Mesh components on the GPU (csrc/meshcomp.hip: bnv_mesh_components, bnv_mesh_filter_components) against the host
functions mesh.connected_components / mesh.remove_small_components, bit for bit: labels, face counts, area float64 bits,
filtered vertex float32 bits, faces."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
import mesh_components_restatement as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = rs.adversarial_cases()


def up(v, f):
    return (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(f, np.int64)).to(DEV))


def assert_same_mesh(got, want):
    gv, gf = got
    assert gv.shape == want.vertices.shape, (gv.shape, want.vertices.shape)
    assert np.array_equal(gv.view(np.uint32), want.vertices.view(np.uint32)), int((gv != want.vertices).sum())
    assert gf.shape == want.faces.shape and np.array_equal(gf, want.faces)


def assert_same_components(got, want):
    labels, n_faces, areas = got
    assert labels.dtype == torch.int32 and n_faces.dtype == torch.int64 and areas.dtype == torch.float64
    assert labels.is_cuda and n_faces.is_cuda and areas.is_cuda
    assert np.array_equal(labels.cpu().numpy(), want[0])
    assert np.array_equal(n_faces.cpu().numpy(), want[1])
    assert np.array_equal(areas.cpu().numpy().view(np.uint64), want[2].view(np.uint64))


def gpu_filter(v, f, **kw):
    from bnv_fusion_amd import mesh as M
    vs, fs = M.remove_small_components_tensors(*up(v, f), **kw)
    assert vs.is_cuda and fs.is_cuda and vs.dtype == torch.float32 and fs.dtype == torch.int64
    return vs.cpu().numpy(), fs.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_adversarial_equals_host(case):
    from bnv_fusion_amd import mesh as M
    _, v, f, filters = case
    assert_same_components(M.connected_components_tensors(*up(v, f)), M.connected_components(M.TriMesh(v, f)))
    for kw in filters:
        assert_same_mesh(gpu_filter(v, f, **kw), M.remove_small_components(M.TriMesh(v, f), **kw))


def test_everything_removed_is_empty():
    v, f = rs.isolated_triangles(300)
    gv, gf = gpu_filter(v, f, min_area=1.0)
    assert gv.shape == (0, 3) and gf.shape == (0, 3)


def test_two_calls_bit_identical():
    from bnv_fusion_amd import mesh as M
    v, f, _ = next(c[1:] for c in CASES if c[0] == "strip_4097_shuffled")
    vt, ft = up(v, f)
    a, b = M.connected_components_tensors(vt, ft), M.connected_components_tensors(vt, ft)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))
    v, f, _ = next(c[1:] for c in CASES if c[0] == "fans_all_criteria")
    vt, ft = up(v, f)
    a = M.remove_small_components_tensors(vt, ft, min_area=0.3, min_faces=5, keep_largest=4)
    b = M.remove_small_components_tensors(vt, ft, min_area=0.3, min_faces=5, keep_largest=4)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_trimesh_entry_point():
    from bnv_fusion_amd import mesh as M
    v, f = rs.sphere_and_strays()
    got = M.remove_small_components_gpu(M.TriMesh(v, f), min_area=0.01, min_faces=3, keep_largest=3, device=DEV)
    assert_same_mesh((got.vertices, got.faces),
                     M.remove_small_components(M.TriMesh(v, f), min_area=0.01, min_faces=3, keep_largest=3))


def test_post_process_surface_threshold_equals_host():
    from bnv_fusion_amd import mesh as M
    v, f = rs.sphere_and_strays()
    vs, fs = v[f.reshape(-1)], np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)       # unwelded
    areas = np.sort(M.connected_components(M.post_process_mesh(M.TriMesh(vs, fs), 0.025))[2])
    vt, ft = up(vs, fs)
    for s in (float(areas[0]), float(areas[1] + areas[2]) / 2, float(areas[3]) * 2):
        got = M.post_process_mesh_tensors(vt, ft, 0.025, surface_threshold=s)
        assert_same_mesh((got[0].cpu().numpy(), got[1].cpu().numpy()),
                         M.post_process_mesh(M.TriMesh(vs, fs), 0.025, surface_threshold=s))
    got = M.post_process_mesh_gpu(M.TriMesh(vs, fs), 0.025, device=DEV, surface_threshold=float(areas[1]))
    assert_same_mesh((got.vertices, got.faces),
                     M.post_process_mesh(M.TriMesh(vs, fs), 0.025, surface_threshold=float(areas[1])))
    a = M.post_process_mesh_tensors(vt, ft, 0.025, surface_threshold=None)
    b = M.post_process_mesh_tensors(vt, ft, 0.025)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert_same_mesh((a[0].cpu().numpy(), a[1].cpu().numpy()), M.post_process_mesh(M.TriMesh(vs, fs), 0.025))


def test_invalid_input_raises():
    from bnv_fusion_amd import mesh as M
    v = torch.rand((10, 3), device=DEV)
    f = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int64, device=DEV)
    bad = [(v.cpu(), f), (v, f.cpu()), (v.double(), f), (v, f.int()), (v[:, :2], f), (v, f[:, :2]),
           (v, f + 8), (v, f - 1)]
    nan = v.clone()
    nan[4, 1] = float("nan")
    inf = v.clone()
    inf[9, 0] = float("inf")                                 # an unreferenced vertex: refused all the same
    bad += [(nan, f), (inf, f), (v[:0], f)]
    for vv, ff in bad:
        with pytest.raises(ValueError):
            M.connected_components_tensors(vv, ff)
        with pytest.raises(ValueError):
            M.remove_small_components_tensors(vv, ff, min_area=0.01)
    for kw in (dict(min_area=-1.0), dict(min_area=float("nan")), dict(min_area=float("inf")), dict(min_faces=-1),
               dict(keep_largest=0)):
        with pytest.raises(ValueError):
            M.remove_small_components_tensors(v, f, **kw)
    for s in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            M.post_process_mesh_tensors(v, f, 0.01, surface_threshold=s)


def test_c_entries_report_invalid_input():
    """The device's own refusal, below the Python checks: count = -1 and counts = {-1, -1} for a face index out of
    range, a non-finite vertex (referenced or not) and an area of 2^12; valid input right after gives the counts."""
    import ctypes as C
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    v = torch.rand((10, 3), device=DEV)
    f = torch.tensor([[0, 1, 2], [3, 4, 5], [2, 1, 6]], dtype=torch.int64, device=DEV)
    nan = v.clone()
    nan[9, 2] = float("nan")
    big = torch.tensor([[0, 0, 0], [128, 0, 0], [0, 64, 0]] + [[0, 0, 0]] * 7, dtype=torch.float32, device=DEV)
    f_hi, f_lo = f.clone(), f.clone()
    f_hi[1, 2], f_lo[2, 0] = 10, -1
    for vv, ff, want in ((v, f_hi, -1), (v, f_lo, -1), (nan, f, -1), (big, f, -1), (v, f, 2)):
        V, T = int(vv.shape[0]), int(ff.shape[0])
        need = C.c_int64()
        assert lib.bnv_mesh_components_workspace_bytes(V, T, C.byref(need)) == 0
        ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
        labels = torch.empty(T, dtype=torch.int32, device=DEV)
        n_faces = torch.empty(T, dtype=torch.int64, device=DEV)
        areas = torch.empty(T, dtype=torch.float64, device=DEV)
        count = torch.empty(1, dtype=torch.int64, device=DEV)
        assert lib.bnv_mesh_components(_lib.ptr(vv), V, _lib.ptr(ff), T, _lib.ptr(ws), need.value, _lib.ptr(labels),
                                       _lib.ptr(n_faces), _lib.ptr(areas), _lib.ptr(count), _lib.stream_ptr()) == 0
        assert count.item() == want
        v_out, f_out = torch.empty_like(vv), torch.empty_like(ff)
        counts = torch.empty(2, dtype=torch.int64, device=DEV)
        assert lib.bnv_mesh_filter_components(_lib.ptr(vv), V, _lib.ptr(ff), T, C.c_double(0.0), 0, 0, _lib.ptr(ws),
                                              need.value, _lib.ptr(v_out), _lib.ptr(f_out), _lib.ptr(counts),
                                              _lib.stream_ptr()) == 0
        assert counts.tolist() == ([-1, -1] if want < 0 else [7, 3])


def test_total_area_limit_raises():
    from bnv_fusion_amd import mesh as M
    big = np.array([[0, 0, 0], [128, 0, 0], [0, 64, 0]], np.float32)                        # area exactly 2^12
    one = np.array([[0, 1, 2]], np.int64)
    for fn in (M.connected_components_tensors, M.remove_small_components_tensors):
        with pytest.raises(ValueError, match="2\\^12"):
            fn(*up(big, one))
    unit = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0]], np.float32)                          # area 1, 4096 times
    many = np.tile(one, (4096, 1))
    for fn in (M.connected_components_tensors, M.remove_small_components_tensors):
        with pytest.raises(ValueError, match="2\\^12"):
            fn(*up(unit, many))
    assert_same_components(M.connected_components_tensors(*up(unit, many[:4095])),
                           M.connected_components(M.TriMesh(unit, many[:4095])))


def test_room_sweep_extract_mesh_min_component_area():
    import bnv_fusion_amd as bnv
    from bnv_fusion_amd import evaluate, sequence
    from bnv_fusion_amd import mesh as M
    dims, voxel, scale = sequence.DIMS[256]
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    nm = bnv.NeuralMap(np.array([dims] * 3), voxel, model, device=DEV)
    for fr in sequence.sweep_frames(range(0, 120, 2), scale=scale, device=DEV):
        nm.integrate(fr)
    eps = nm.voxel_size / 4
    a = 0.1 * scale * scale                                  # the reference's 0.1 m^2, in the half-scale scene
    with pytest.raises(ValueError, match="post_process"):
        nm.extract_mesh(min_component_area=a)
    post = M.post_process_mesh(nm.extract_mesh(), eps)
    want = M.remove_small_components(post, min_area=a)
    got = nm.extract_mesh(post_process=eps, min_component_area=a)
    assert_same_mesh((got.vertices, got.faces), want)
    # what the specification guarantees for any mesh
    labels, n_faces, areas = M.connected_components(post)
    assert_same_components(M.connected_components_tensors(*up(post.vertices, post.faces)), (labels, n_faces, areas))
    kept = areas >= a
    fk = kept[labels]
    assert np.array_equal(post.vertices[post.faces[fk]].view(np.uint32), got.vertices[got.faces].view(np.uint32))
    largest = int(np.argmax(areas))
    assert areas[largest] >= a and kept[largest]             # a room of metres against 0.025 m^2
    q, q_got = M._face_area_units(post.vertices, post.faces), M._face_area_units(got.vertices, got.faces)
    assert int(q_got.sum()) + int(q[~fk].sum()) == int(q.sum())          # kept + removed = total, in 2^-50 units
    hist = np.histogram(areas, bins=[0, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1, 1e3])[0]
    print(f"room sweep 256: C = {len(areas)}, largest share = {areas[largest] / areas.sum():.6f}, removed "
          f"{int((~fk).sum())} of {len(fk)} faces, {areas[~kept].sum():.6f} of {areas.sum():.6f} m^2; "
          f"areas per decade from 1e-6: {hist.tolist()}")
    gt = sequence.gt_mesh(scale)
    for name, m in (("without the filter", post), ("with the filter   ", got)):
        res = evaluate.evaluate_meshes(m, gt, generator=torch.Generator(device=DEV).manual_seed(0), device=DEV)
        print(f"room sweep 256, {name}:", evaluate.summary_line(res))
