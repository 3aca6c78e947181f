"""Checks of batched graph construction (equidock_public_amd.dock.protein_graphs_batch, eqd_dock_graph_* of
libequidock_dock.so) shared by the simulator tests (tests/test_dock_graph_sim.py) and the GPU tests
(tests/test_dock_graph_gpu.py).  Both libraries must be loaded by the caller: the per-protein path
(featurize.protein_graph, libequidock_hip.so) is what the batched path is compared with bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from equidock_public_amd import _lib, dock as DK, featurize as FZ
from tests import dock_common as dc
from tests.parity_common import _residues_from_fixture

KEYS = ('x', 'res_feat', 'mu_r_norm', 'src', 'dst', 'he')
SIM_CASES = ('graph_case', 'graph_case_tiny', 'graph_case_pair300')
GPU_CASES = SIM_CASES + ('graph_case_big',)
PRUNE_ENV = 'EQD_DOCK_GRAPH_PRUNE'


def fixture_proteins(names):
    """The ligand and the receptor of every fixture as {'tag', 'residues', 'bound_ca', 'ref', 'stride'}: the inputs of
    featurize.protein_graph after preprocess_unbound_bound, and the reference's recorded graph."""
    out = []
    for name in names:
        z = np.load(os.path.join(dc.GOLDEN, f'{name}.npz'))
        lig, rec, lig_ca, rec_ca = FZ.preprocess_unbound_bound(_residues_from_fixture(z, 'lig_in_'),
                                                               _residues_from_fixture(z, 'rec_in_'), inference=True)
        assert float(z['cutoff']) == 30.0 and int(z['max_neighbor']) == 10
        stride = int(z['he_stride']) if 'he_stride' in z.files else 1
        for side, res, ca in (('lig', lig, lig_ca), ('rec', rec, rec_ca)):
            out.append({'tag': f'{name}/{side}', 'residues': res, 'bound_ca': ca, 'stride': stride,
                        'ref': {k: z[f'{side}_{k}'] for k in ('src', 'dst', 'he', 'x', 'mu', 'res')}})
    return out


def batch_of(prots, dev, cutoff=30.0, K=10):
    return DK.protein_graphs_batch([(p['residues'], p['bound_ca']) for p in prots], cutoff, K, dev)


def same_graph_bits(a, b, what):
    """Every output tensor of two graphs of one protein: same dtype, shape and bits (device tensors); and, where the
    batched path gave host views, those hold the same bytes as its device tensors."""
    for k in KEYS:
        ta, tb = a[k], b[k]
        assert ta.dtype == tb.dtype and ta.shape == tb.shape, (what, k, ta.dtype, tb.dtype, tuple(ta.shape), tuple(tb.shape))
        assert torch.equal(ta.cpu(), tb.cpu()), f'{what}: {k} differs'
        assert ta.cpu().numpy().tobytes() == tb.cpu().numpy().tobytes(), f'{what}: {k} differs in bits'
    for g in (a, b):
        if 'host' in g:
            for k in KEYS:
                h = g['host'][k]
                assert isinstance(h, np.ndarray) and h.dtype == g[k].cpu().numpy().dtype and h.shape == tuple(g[k].shape)
                assert h.tobytes() == g[k].cpu().numpy().tobytes(), f'{what}: host view of {k}'


def check_reference_graphs(dev, names):
    """1. all proteins of the fixtures in ONE batch at the fixtures' cutoff 30 and K 10 against the reference's recorded
    graphs: int32 endpoints exactly, features within the existing 1e-6 bound"""
    prots = fixture_proteins(names)
    out = batch_of(prots, dev)
    assert len(out) == len(prots)
    for p, g in zip(prots, out):
        ref, tag = p['ref'], p['tag']
        assert g['src'].dtype == torch.int32 and g['dst'].dtype == torch.int32
        assert ref['src'].dtype == np.int32 and ref['dst'].dtype == np.int32
        assert np.array_equal(g['src'].cpu().numpy(), ref['src']), f'{tag}: source indices differ from the reference'
        assert np.array_equal(g['dst'].cpu().numpy(), ref['dst']), f'{tag}: destination indices differ from the reference'
        assert np.array_equal(g['res_feat'].cpu().numpy(), ref['res'])
        dc.close(g['he'][::p['stride']], ref['he'], 1e-6, f'{tag}: edge features')
        dc.close(g['x'], ref['x'], 1e-6, f'{tag}: x')
        dc.close(g['mu_r_norm'], ref['mu'], 1e-6, f'{tag}: mu_r_norm')
        dc.close(g['host']['he'][::p['stride']], ref['he'], 1e-6, f'{tag}: edge features (host view)')
    return out


def per_protein(p, dev, cutoff, K):
    return FZ.protein_graph(p['residues'], p['bound_ca'], cutoff, K, dev)


def check_against_per_protein(dev, names):
    """2. every output tensor of every protein bit-equal to featurize.protein_graph on the same inputs: cutoff 30 / K 10,
    cutoff 9 / K 10 (the np.where branch: rows with fewer than K candidates), K = 1 and K = 64"""
    prots = fixture_proteins(names)
    for cutoff, K in ((30.0, 10), (9.0, 10), (30.0, 1), (30.0, 64)):
        use, single = [], []
        for p in prots:
            try:
                single.append(per_protein(p, dev, cutoff, K))
                use.append(p)
            except ValueError:        # cutoff 9 isolates a residue of this protein: the per-protein path refuses it too
                assert cutoff == 9.0, (p['tag'], cutoff, K)
        assert len(use) >= 2, f'cutoff {cutoff}: only {len(use)} fixture proteins have no isolated residue'
        out = batch_of(use, dev, cutoff, K)
        short = 0
        for p, s, g in zip(use, single, out):
            same_graph_bits(g, s, f"{p['tag']} at cutoff {cutoff}, K {K}: batched vs per-protein")
            n = len(p['residues'])
            short += int((np.bincount(g['dst'].cpu().numpy(), minlength=n) < min(K, n - 1)).sum())
        if cutoff == 9.0:
            assert short > 0, 'cutoff 9 left no row with fewer than K candidates: the np.where branch was not covered'
        if K == 64:
            assert any(len(p['residues']) > 65 for p in use) and any(len(p['residues']) <= 64 for p in use)


def check_composition(dev, names, target='graph_case/rec'):
    """3. a protein gives the same bits alone, first, last and in a permuted batch of all fixture proteins; two runs of
    the same batch give the same bits"""
    prots = fixture_proteins(names)
    t = [i for i, p in enumerate(prots) if p['tag'] == target][0]
    others = [p for i, p in enumerate(prots) if i != t]
    alone = batch_of([prots[t]], dev)[0]
    first = batch_of([prots[t]] + others, dev)
    last = batch_of(others + [prots[t]], dev)
    same_graph_bits(alone, first[0], f'{target}: alone vs first')
    same_graph_bits(alone, last[-1], f'{target}: alone vs last')
    perm = np.random.default_rng(5).permutation(len(prots))
    assert not np.array_equal(perm, np.arange(len(prots)))
    mixed = batch_of([prots[i] for i in perm], dev)
    same_graph_bits(alone, mixed[int(np.nonzero(perm == t)[0][0])], f'{target}: alone vs permuted batch')
    # every other protein too: its place in `first` vs its place in the permuted batch
    for k, p in enumerate(others):
        i = [q['tag'] for q in prots].index(p['tag'])
        same_graph_bits(first[1 + k], mixed[int(np.nonzero(perm == i)[0][0])], f"{p['tag']}: two batch positions")
    again = batch_of([prots[i] for i in perm], dev)
    for k, (a, b) in enumerate(zip(mixed, again)):
        same_graph_bits(a, b, f'run to run, position {k}')


def check_pruning(dev, name, expect_pruned, monkeypatch):
    """4. with the switch on and off every output is bit-equal; the exported pruned-pair count is > 0 (pair300, big) or
    0 (tiny) with it on, 0 with it off"""
    prots = fixture_proteins([name])
    monkeypatch.setenv(PRUNE_ENV, '1')
    on = batch_of(prots, dev)
    st_on = dict(DK.last_graph_stats)
    monkeypatch.setenv(PRUNE_ENV, '0')
    off = batch_of(prots, dev)
    st_off = dict(DK.last_graph_stats)
    monkeypatch.delenv(PRUNE_ENV)
    assert st_on['pruning'] is True and st_off['pruning'] is False and DK.graph_pruning_enabled()
    for p, a, b in zip(prots, on, off):
        same_graph_bits(a, b, f"{p['tag']}: pruning on vs off")
    assert st_off['pruned_pairs'] == 0, st_off
    assert st_on['pairs'] == sum(len(p['residues']) * (len(p['residues']) - 1) // 2 for p in prots)
    if expect_pruned:
        assert 0 < st_on['pruned_pairs'] < st_on['pairs'], st_on
    else:
        assert st_on['pruned_pairs'] == 0, st_on
    return st_on


def merged_long_residue(residues, start, count):
    """`count` neighbouring residues from `start` merged into ONE residue that keeps the first one's N / CA / C; the same
    atoms of the others are renamed, so that the residue still has exactly one of each."""
    group = residues[start:start + count]
    names, elements, coords = [], [], []
    for k, r in enumerate(group):
        for a, e in zip(r.atom_names, r.elements):
            names.append(a + 'X' if k > 0 and a in ('N', 'CA', 'C') else a)
            elements.append(e)
        coords.append(r.coords)
    first = group[0]
    big = FZ.Residue(first.chain, first.number, first.resname, names, elements, np.concatenate(coords, 0))
    return list(residues[:start]) + [big] + list(residues[start + count:]), big


def check_long_residue(dev):
    """5. a residue of more than 64 atoms (the global-memory path of the distance kernel) is bit-equal to the per-protein
    path, in a batch behind another protein"""
    prots = fixture_proteins(['graph_case'])
    rec = prots[1]
    residues, big = merged_long_residue(rec['residues'], 10, 12)
    assert len(big.coords) > 64, len(big.coords)
    assert len(FZ.filter_residues(residues)) == len(residues)
    long_p = {'tag': 'graph_case/rec with a long residue', 'residues': residues, 'bound_ca': FZ.alpha_carbon_array(residues)}
    single = per_protein(long_p, dev, 30.0, 10)
    out = batch_of([prots[0], long_p], dev)
    same_graph_bits(out[1], single, 'long residue: batched vs per-protein')
    same_graph_bits(out[0], per_protein(prots[0], dev, 30.0, 10), 'the protein in front of it')
    return len(big.coords)


def check_errors(dev):
    """6. isolated residue in the second protein -> ValueError naming index 1; K = 0 / 65; invalid offsets -> the workspace
    query returns 0 with a message; an empty list -> []"""
    prots = fixture_proteins(['graph_case'])
    lig, rec = prots
    far = [FZ.Residue(r.chain, r.number, r.resname, r.atom_names, r.elements, r.coords.copy()) for r in rec['residues']]
    far[7].coords += np.float32(500.0)
    lonely = {'residues': far, 'bound_ca': FZ.alpha_carbon_array(far)}
    with pytest.raises(ValueError, match='no neighbour'):
        per_protein(lonely, dev, 30.0, 10)
    with pytest.raises(ValueError, match=r'protein 1 of the batch: residue 7 has no neighbour'):
        batch_of([lig, lonely], dev)
    with pytest.raises(ValueError, match=r'protein 0 of the batch'):
        batch_of([lonely, lig], dev)
    for K in (0, 65):
        with pytest.raises(ValueError, match='max_neighbor'):
            batch_of([lig], dev, K=K)
    with pytest.raises(ValueError, match='only 1 residue'):
        DK.protein_graphs_batch([(lig['residues'], lig['bound_ca']), (lig['residues'][:1], lig['bound_ca'][:1])], 30.0, 10, dev)
    assert DK.protein_graphs_batch([], 30.0, 10, dev) == []
    lib = DK.load_dock_library()
    assert lib.eqd_dock_graph_abi() == 1 and lib.eqd_dock_abi_version() == 1

    def ws_bytes(res_off, atom_off, K=10):
        r, a = (np.ascontiguousarray(np.asarray(v, dtype=np.int32)) for v in (res_off, atom_off))
        return lib.eqd_dock_graph_workspace_bytes(len(r) - 1, r.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), K)

    assert ws_bytes([0, 4, 9], [0, 40, 90]) > 0
    assert ws_bytes([0, 6, 4], [0, 40, 90]) == 0                       # non-monotone
    assert b'protein 1 has -2 residues' in lib.eqd_dock_last_error()
    assert ws_bytes([0, 4, 4], [0, 40, 90]) == 0                       # an empty protein
    assert ws_bytes([1, 4, 9], [0, 40, 90]) == 0                       # does not start at 0
    assert ws_bytes([0, 4, 9], [0, 3, 90]) == 0                        # fewer atoms than residues
    assert ws_bytes([0, 4, 9], [0, 40, 90], K=65) == 0 and b'max_neighbor 65' in lib.eqd_dock_last_error()
    assert ws_bytes([0, 70000], [0, 700000]) == 0 and b'32-bit' in lib.eqd_dock_last_error()      # 4.9e9 distance entries
    # a refused init writes nothing
    wsb = ws_bytes([0, 4, 9], [0, 40, 90])
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    r, a = np.asarray([0, 4, 9], dtype=np.int32), np.asarray([0, 40, 90], dtype=np.int32)
    rc = lib.eqd_dock_graph_init(2, r.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), 10, C.c_void_p(ws.data_ptr()),
                                 C.c_size_t(64), DK._stream(dev))
    assert rc == 4 and b'workspace too small' in lib.eqd_dock_last_error()
    assert bool((ws.cpu() == 0).all())


def check_pipeline(dev, names, max_it=5, check_every=2):
    """7. dock_complexes with batched_graphs=True and False on the real fixture complexes (seeded weights): bit-equal"""
    net, _, _ = dc.seeded_net(dev)
    residues = [dc.fixture_residues(n) for n in names]
    a = DK.dock_complexes(net, residues, remove_clashes=True, max_it=max_it, check_every=check_every, device=dev,
                          batched_graphs=True)
    b = DK.dock_complexes(net, residues, remove_clashes=True, max_it=max_it, check_every=check_every, device=dev,
                          batched_graphs=False)
    assert len(a) == len(b) == len(names)
    for name, x, y in zip(names, a, b):
        for k in ('rotation', 'translation'):
            assert x[k].dtype == y[k].dtype and x[k].tobytes() == y[k].tobytes(), (name, k, x[k], y[k])
        for k in ('ligand_atoms_docked', 'ligand_atoms'):
            assert x[k].dtype == y[k].dtype and torch.equal(x[k].cpu(), y[k].cpu()), (name, k)
        assert x['clash_iterations'] == y['clash_iterations'] >= 1, (name, x['clash_iterations'], y['clash_iterations'])
        assert np.float32(x['clash_loss']).tobytes() == np.float32(y['clash_loss']).tobytes(), (name, x['clash_loss'], y['clash_loss'])
        assert x['batch_seconds']['graphs'] > 0 and y['batch_seconds']['graphs'] > 0
    return a
