"""Checks of batched docking inference (equidock_public_amd.dock, libequidock_dock.so) shared by the simulator tests
(tests/test_dock_sim.py) and the GPU tests (tests/test_dock_gpu.py), and the simulator build of csrc_dock/."""
import ctypes as C
import fcntl
import glob
import os
import subprocess

import numpy as np
import torch

from equidock_public_amd import dock as DK, inference as INF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
HOSTSIM = os.path.join(ROOT, 'tests', 'hostsim')
SIM_OUT = os.path.join(HOSTSIM, 'build', 'dock')
SIM_LIB = os.path.join(SIM_OUT, 'libeqd_dock_hostsim.so')
CXX = '/opt/rocm/lib/llvm/bin/clang++'
SIM_FLAGS = ['-O2', '-g', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden', '-I', HOSTSIM,
             '-Wno-unknown-attributes', '-Wno-ignored-attributes', '-Wno-unused-function', '-Wno-unused-variable']


def build_sim():
    """csrc_dock/*.hip for x86 against the host simulator (tests/hostsim/hip/hip_runtime.h + hostsim.cpp) ->
    tests/hostsim/build/dock/libeqd_dock_hostsim.so (a library of its own, apart from tests/hostsim/build.py's)."""
    os.makedirs(SIM_OUT, exist_ok=True)
    srcs = sorted(glob.glob(os.path.join(ROOT, 'equidock_public_amd', 'csrc_dock', '*.hip'))) + [os.path.join(HOSTSIM, 'hostsim.cpp')]
    deps = srcs + [os.path.join(ROOT, 'equidock_public_amd', 'csrc', 'eqd_common.h'), os.path.join(HOSTSIM, 'hip', 'hip_runtime.h'),
                   os.path.join(ROOT, 'include', 'equidock_hip.h'), os.path.join(ROOT, 'include', 'equidock_dock.h')]
    with open(os.path.join(SIM_OUT, '.lock'), 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not os.path.exists(SIM_LIB) or any(os.path.getmtime(d) > os.path.getmtime(SIM_LIB) for d in deps):
                cmd = [CXX] + SIM_FLAGS + ['-shared', '-x', 'c++'] + srcs + ['-o', SIM_LIB]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    raise RuntimeError(' '.join(cmd) + '\n' + r.stdout + r.stderr)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return SIM_LIB


def close(got, ref, tol, what=''):
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    ref = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, dtype=np.float64)
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} > {tol:g} * {scale:.3g}"


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def fixture_atoms(name):
    z = np.load(os.path.join(GOLDEN, f'{name}.npz'))
    return z['lig_in_atoms'], z['rec_in_atoms']


def same_bits(a, b, what):
    assert a['iterations'] == b['iterations'], (what, a['iterations'], b['iterations'])
    assert np.float32(a['loss']).tobytes() == np.float32(b['loss']).tobytes(), (what, a['loss'], b['loss'])
    assert a['euler'].tobytes() == b['euler'].tobytes(), (what, a['euler'], b['euler'])
    assert a['translation'].tobytes() == b['translation'].tobytes(), (what, a['translation'], b['translation'])
    assert torch.equal(a['positions'].cpu(), b['positions'].cpu()), what


def check_reference_trajectories(dev, extra=()):
    """inference_case a (cap 300), b (converges; the reference stops after 1 199 iterations) and c (cap 2 000) in ONE
    batch with per-complex caps, against the trajectories recorded from the reference (oracle/make_golden_inference.py),
    with the tolerances of parity_common.check_inference_postprocessing.  `extra`: more (ligand, receptor, cap) complexes
    riding in the same batch (their results must be finite and respect the cap)."""
    z = np.load(os.path.join(GOLDEN, 'inference_case.npz'))
    tags = ('a', 'b', 'c')
    ligs = [_t(z[t + '_lig'], dev) for t in tags] + [_t(e[0], dev) for e in extra]
    recs = [_t(z[t + '_rec'], dev) for t in tags] + [_t(e[1], dev) for e in extra]
    caps = [int(z[t + '_max_it']) for t in tags] + [int(e[2]) for e in extra]
    out = DK.remove_clashes_batch(ligs, recs, max_it=caps, check_every=100)
    a, b, c = out[:3]
    assert a['iterations'] == int(z['a_it']) == caps[0]
    close(a['positions'], z['a_pos'], 1e-4, 'a: ligand atoms after 300 iterations')
    close(a['euler'], z['a_euler'], 1e-4, 'a: euler angles')
    close(a['translation'], z['a_trans'], 1e-4, 'a: translation')
    it_ref = int(z['b_it'])
    assert it_ref < caps[1] and abs(b['iterations'] - it_ref) <= 3, (b['iterations'], it_ref)
    assert b['loss'] <= 0.5, b['loss']
    close(b['positions'], z['b_pos'], 5e-4, 'b: converged ligand atoms')
    assert c['iterations'] == int(z['c_it']) == caps[2]
    ref_c = float(z['c_losses'][-1])
    assert abs(c['loss'] - ref_c) <= 3e-2 * ref_c, (c['loss'], ref_c)
    for r, lig in zip(out, ligs):
        R = INF.get_rot_mat(torch.from_numpy(r['euler']))
        close(r['positions'], INF.apply_rigid(R, r['translation'], lig.cpu()), 1e-5, 'positions vs (euler, t)')
    for r, cap in zip(out[3:], caps[3:]):
        assert 1 <= r['iterations'] <= cap and np.isfinite(r['loss']) and torch.isfinite(r['positions']).all()
    return out


def check_batch_invariance(dev, complexes, caps, runs=1):
    """Every complex's euler, translation, iterations, loss and positions are bit-identical alone, in the batch, in the
    batch in reversed order, and (runs > 1) from run to run."""
    ligs = [_t(l, dev) for l, _ in complexes]
    recs = [_t(r, dev) for _, r in complexes]
    n = len(complexes)
    alone = [DK.remove_clashes_batch([ligs[i]], [recs[i]], max_it=[caps[i]], check_every=7)[0] for i in range(n)]
    together = DK.remove_clashes_batch(ligs, recs, max_it=caps, check_every=7)
    rev = DK.remove_clashes_batch(ligs[::-1], recs[::-1], max_it=caps[::-1], check_every=7)[::-1]
    for i in range(n):
        same_bits(alone[i], together[i], f'complex {i}: alone vs in the batch')
        same_bits(alone[i], rev[i], f'complex {i}: alone vs in the reversed batch')
    for _ in range(runs - 1):
        again = DK.remove_clashes_batch(ligs, recs, max_it=caps, check_every=7)
        for i in range(n):
            same_bits(together[i], again[i], f'complex {i}: run to run')
    return together


def check_validation_errors(dev):
    """Host-side checks before any launch: mismatched list lengths (Python), an empty complex and non-monotone offsets
    (the library: an error code and message, nothing launched)."""
    import pytest
    lig, rec = torch.zeros(4, 3, device=dev), torch.ones(5, 3, device=dev)
    with pytest.raises(ValueError, match='ligands for'):
        DK.remove_clashes_batch([lig, lig], [rec])
    with pytest.raises(ValueError, match='max_it'):
        DK.remove_clashes_batch([lig], [rec], max_it=[10, 10])
    with pytest.raises(RuntimeError, match='complex 1 has 0 ligand'):
        DK.remove_clashes_batch([lig, lig[:0]], [rec, rec])
    lib = DK.load_dock_library()

    def offs(v):
        return np.ascontiguousarray(np.asarray(v, dtype=np.int32))

    def ws_bytes(lo, ro, n):
        return lib.eqd_dock_clash_workspace_bytes(n, lo.ctypes.data_as(C.c_void_p), ro.ctypes.data_as(C.c_void_p))

    good_l, good_r = offs([0, 4, 9]), offs([0, 5, 7])
    assert ws_bytes(good_l, good_r, 2) > 0
    bad = offs([0, 6, 4])                                              # non-monotone
    assert ws_bytes(bad, good_r, 2) == 0
    assert b'complex 1 has -2 ligand' in lib.eqd_dock_last_error()
    assert ws_bytes(offs([0, 4, 4]), good_r, 2) == 0                   # empty ligand
    assert ws_bytes(offs([1, 4, 9]), good_r, 2) == 0                   # does not start at 0
    caps = offs([5, 5])
    states = torch.full((2 * C.sizeof(INF.EqdClashState),), 7, dtype=torch.uint8, device=dev)
    n_done = torch.full((1,), 3, dtype=torch.int32, device=dev)
    wsb = ws_bytes(good_l, good_r, 2)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    st = DK._stream(dev)

    def init(lo, ro, size):
        return lib.eqd_dock_clash_init(2, lo.ctypes.data_as(C.c_void_p), ro.ctypes.data_as(C.c_void_p),
                                       caps.ctypes.data_as(C.c_void_p), C.c_void_p(states.data_ptr()),
                                       C.c_void_p(n_done.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_size_t(size), st)

    assert init(bad, good_r, wsb) == 2
    assert init(good_l, offs([0, 5, 5]), wsb) == 2
    assert init(good_l, good_r, 64) == 4 and b'workspace too small' in lib.eqd_dock_last_error()
    it_rc = lib.eqd_dock_clash_iterations(1, 2, bad.ctypes.data_as(C.c_void_p), good_r.ctypes.data_as(C.c_void_p),
                                          C.c_void_p(lig.data_ptr()), C.c_void_p(rec.data_ptr()), C.c_float(8.0),
                                          C.c_float(8.0), C.c_float(0.5), C.c_void_p(states.data_ptr()),
                                          C.c_void_p(n_done.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_size_t(wsb), st)
    assert it_rc == 2
    # nothing was written by the refused calls
    assert int(n_done.cpu()[0]) == 3 and bool((states.cpu() == 7).all()) and bool((ws.cpu() == 0).all())


# ---- end to end ---------------------------------------------------------------------------------------------------
REAL = ('graph_case', 'graph_case_pair300', 'graph_case_big')


def fixture_residues(name):
    from tests.parity_common import _residues_from_fixture
    z = np.load(os.path.join(GOLDEN, f'{name}.npz'))
    return _residues_from_fixture(z, 'lig_in_'), _residues_from_fixture(z, 'rec_in_')


def write_pdb(residues, path):
    """ATOM records in the fixed columns featurize.read_pdb_residues / inference.read_pdb_atoms read."""
    k = 1
    with open(path, 'w') as f:
        for r in residues:
            for name, el, (x, y, z) in zip(r.atom_names, r.elements, r.coords):
                nm = f" {name:<3}" if len(name) < 4 else name
                f.write(f"ATOM  {k:5d} {nm:4s} {r.resname:>3s} {r.chain:1s}{r.number:4d}    "
                        f"{x:8.3f}{y:8.3f}{z:8.3f}{1.0:6.2f}{0.0:6.2f}          {el:>2s}\n")
                k += 1
        f.write("END\n")


def seeded_net(dev, seed=7):
    """The DB5.5 published configuration (5 shared layers) with config.seeded_state_dict weights."""
    from equidock_public_amd import config, model
    args = config.published_args(iegmn_n_lays=5, shared_layers=True, skip_weight_h=0.5)
    sd = config.seeded_state_dict(args, seed)
    net = model.Rigid_Body_Docking_Net(dict(args, device=dev)).to(dev)
    net.load_state_dict(sd)
    return net.eval(), args, sd


def single_complex_pipeline(net, lig_res, rec_res, dev):
    """The steps of parity_common.check_inference_pipeline for one complex: (R, t)."""
    from equidock_public_amd import featurize as FZ, graph as G
    lig, rec, lig_ca, rec_ca = FZ.preprocess_unbound_bound(lig_res, rec_res, inference=True)
    gl, gr = FZ.protein_to_graph_unbound_bound(lig, rec, lig_ca, rec_ca, cutoff=30.0, max_neighbor=10, device=dev)
    batch = G.batch_pairs([(dict(gl, new_x=gl['x']), gr)]).to(dev)
    with torch.no_grad():
        _, _, _, rot, tr = net(batch, epoch=0)
    return rot[0].cpu().numpy(), tr[0].cpu().numpy().reshape(3)
