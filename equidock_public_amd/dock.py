"""Batched docking inference: src/inference_rigid.py's loop over a directory of complexes (:85-245) for N complexes at once.

    graphs of all complexes in one device pass (protein_graphs_batch)  ->  one batched eval forward per chunk
    ->  apply_rigid to each ligand's atoms
    ->  remove_clashes_batch: clash removal of ALL complexes in one device loop (libequidock_dock.so), each stopping on
        its own  ->  with ground truth: ligand / complex / interface RMSD of ALL complexes in one device pass
        (rmsd_metrics_batch)  ->  PDB files and the CRMSD / IRMSD summary

Evaluation passes over every heavy atom, one batched device pass each: `pose_quality_batch` (fnat, LRMSD, backbone iRMSD,
DockQ, clashes), `surface_area_batch` (SASA, buried surface area), `lddt_batch` (lDDT, interface lDDT, per-residue scores)
and `residue_depth_batch` (atom and residue depth below the surface, alone and in complex); `surface_feature_analysis` is
src/surface_analysis.py on top of the last one.

`remove_clashes_batch` is `inference.remove_clashes` for a list of complexes: same keys, same stop rule, same meaning;
`rmsd_metrics_batch` / `DeviceMeter` are `inference.rmsd_metrics` + `complex_and_interface_rmsd` /
`inference.Meter_Unbound_Bound` for a list of complexes, results on the device; `dock_complexes` is the Python API, `python -m equidock_public_amd.dock` the command-line counterpart of
inference_rigid.py.  There is no fallback: a missing libequidock_dock.so is an error.
"""
import argparse
import ctypes as C
import glob
import os
import sys
import time

import numpy as np
import torch

from . import _lib, config, featurize as FZ, graph as G, inference as INF

HERE = os.path.dirname(os.path.abspath(__file__))
DOCK_LIB_PATH = os.path.join(HERE, 'libequidock_dock.so')
DOCK_ABI_VERSION = 1
DOCK_GRAPH_ABI = 1
DOCK_METER_ABI = 1
METER_COLS = 8             # EQD_DOCK_METER_COLS
DOCK_QUALITY_ABI = 1
QUALITY_COLS = 16          # EQD_DOCK_QUALITY_COLS
DOCK_EMD_ABI = 1
EMD_MAX_NODES = 2048       # EQD_DOCK_EMD_MAX_NODES
EMD_RESIDENT_CELLS = 8192  # EQD_DOCK_EMD_RESIDENT_CELLS
DOCK_SASA_ABI = 1
SASA_COLS = 12             # EQD_DOCK_SASA_COLS
SASA_MAX_POINTS = 1024     # EQD_DOCK_SASA_MAX_POINTS
DOCK_LDDT_ABI = 1
LDDT_COLS = 16             # EQD_DOCK_LDDT_COLS
LDDT_BLOCK = 64            # EQD_DOCK_LDDT_BLOCK
DOCK_DEPTH_ABI = 1
DEPTH_COLS = 16            # EQD_DOCK_DEPTH_COLS

_dock = None
_dock_is_sim = False


def _declare(lib):
    lib.eqd_dock_abi_version.restype = C.c_int
    lib.eqd_dock_last_error.restype = C.c_char_p
    lib.eqd_dock_is_simulator.restype = C.c_int
    lib.eqd_dock_clash_workspace_bytes.restype = C.c_size_t
    lib.eqd_dock_clash_workspace_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.eqd_dock_clash_init.restype = C.c_int
    lib.eqd_dock_clash_init.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p]
    lib.eqd_dock_clash_iterations.restype = C.c_int
    lib.eqd_dock_clash_iterations.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                              C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_void_p]
    lib.eqd_dock_graph_abi.restype = C.c_int
    lib.eqd_dock_graph_workspace_bytes.restype = C.c_size_t
    lib.eqd_dock_graph_workspace_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.eqd_dock_graph_init.restype = C.c_int
    lib.eqd_dock_graph_init.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eqd_dock_graph_select.restype = C.c_int
    lib.eqd_dock_graph_select.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                          C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eqd_dock_graph_edges.restype = C.c_int
    lib.eqd_dock_graph_edges.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eqd_dock_meter_abi.restype = C.c_int
    lib.eqd_dock_meter_workspace_bytes.restype = C.c_size_t
    lib.eqd_dock_meter_workspace_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.eqd_dock_meter_init.restype = C.c_int
    lib.eqd_dock_meter_init.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eqd_dock_meter_eval.restype = C.c_int
    lib.eqd_dock_meter_eval.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eqd_dock_quality_abi.restype = C.c_int
    lib.eqd_dock_quality_workspace_bytes.restype = C.c_size_t
    lib.eqd_dock_quality_workspace_bytes.argtypes = [C.c_int] + [C.c_void_p] * 4
    lib.eqd_dock_quality_init.restype = C.c_int
    lib.eqd_dock_quality_init.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]
    lib.eqd_dock_quality_eval.restype = C.c_int
    lib.eqd_dock_quality_eval.argtypes = ([C.c_int] + [C.c_void_p] * 12 + [C.c_double] * 3 + [C.c_int, C.c_void_p, C.c_void_p,
                                                                                             C.c_size_t, C.c_void_p])
    lib.eqd_dock_sasa_abi.restype = C.c_int
    lib.eqd_dock_sasa_workspace_bytes.restype = C.c_size_t
    lib.eqd_dock_sasa_workspace_bytes.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int]
    lib.eqd_dock_sasa_init.restype = C.c_int
    lib.eqd_dock_sasa_init.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eqd_dock_sasa_eval.restype = C.c_int
    lib.eqd_dock_sasa_eval.argtypes = ([C.c_int] + [C.c_void_p] * 11 + [C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 6 +
                                       [C.c_size_t, C.c_void_p])
    lib.eqd_dock_lddt_abi.restype = C.c_int
    lib.eqd_dock_lddt_workspace_bytes.restype = C.c_size_t
    lib.eqd_dock_lddt_workspace_bytes.argtypes = [C.c_int] + [C.c_void_p] * 4
    lib.eqd_dock_lddt_init.restype = C.c_int
    lib.eqd_dock_lddt_init.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]
    lib.eqd_dock_lddt_eval.restype = C.c_int
    lib.eqd_dock_lddt_eval.argtypes = ([C.c_int] + [C.c_void_p] * 10 + [C.c_double, C.c_void_p, C.c_int] + [C.c_void_p] * 6 +
                                       [C.c_size_t, C.c_void_p])
    lib.eqd_dock_depth_abi.restype = C.c_int
    lib.eqd_dock_depth_workspace_bytes.restype = C.c_size_t
    lib.eqd_dock_depth_workspace_bytes.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int]
    lib.eqd_dock_depth_init.restype = C.c_int
    lib.eqd_dock_depth_init.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eqd_dock_depth_eval.restype = C.c_int
    lib.eqd_dock_depth_eval.argtypes = ([C.c_int] + [C.c_void_p] * 13 + [C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 6 +
                                        [C.c_size_t, C.c_void_p])
    lib.eqd_dock_emd_abi.restype = C.c_int
    lib.eqd_dock_emd_workspace_bytes.restype = C.c_size_t
    lib.eqd_dock_emd_workspace_bytes.argtypes = [C.c_int, C.c_void_p, C.c_int]
    lib.eqd_dock_emd_init.restype = C.c_int
    lib.eqd_dock_emd_init.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eqd_dock_emd_solve.restype = C.c_int
    lib.eqd_dock_emd_solve.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_size_t, C.c_void_p]


def _bind(path):
    global _dock, _dock_is_sim
    lib = C.CDLL(path)
    _declare(lib)
    if lib.eqd_dock_abi_version() != DOCK_ABI_VERSION:
        raise _lib.EquidockHipError(f"{path}: dock ABI version {lib.eqd_dock_abi_version()} != {DOCK_ABI_VERSION}")
    if lib.eqd_dock_graph_abi() != DOCK_GRAPH_ABI:
        raise _lib.EquidockHipError(f"{path}: dock graph ABI {lib.eqd_dock_graph_abi()} != {DOCK_GRAPH_ABI}")
    if lib.eqd_dock_meter_abi() != DOCK_METER_ABI:
        raise _lib.EquidockHipError(f"{path}: dock meter ABI {lib.eqd_dock_meter_abi()} != {DOCK_METER_ABI}")
    if lib.eqd_dock_quality_abi() != DOCK_QUALITY_ABI:
        raise _lib.EquidockHipError(f"{path}: dock quality ABI {lib.eqd_dock_quality_abi()} != {DOCK_QUALITY_ABI}")
    if lib.eqd_dock_emd_abi() != DOCK_EMD_ABI:
        raise _lib.EquidockHipError(f"{path}: dock EMD ABI {lib.eqd_dock_emd_abi()} != {DOCK_EMD_ABI}")
    if lib.eqd_dock_sasa_abi() != DOCK_SASA_ABI:
        raise _lib.EquidockHipError(f"{path}: dock SASA ABI {lib.eqd_dock_sasa_abi()} != {DOCK_SASA_ABI}")
    if lib.eqd_dock_lddt_abi() != DOCK_LDDT_ABI:
        raise _lib.EquidockHipError(f"{path}: dock lDDT ABI {lib.eqd_dock_lddt_abi()} != {DOCK_LDDT_ABI}")
    if lib.eqd_dock_depth_abi() != DOCK_DEPTH_ABI:
        raise _lib.EquidockHipError(f"{path}: dock depth ABI {lib.eqd_dock_depth_abi()} != {DOCK_DEPTH_ABI}")
    _dock, _dock_is_sim = lib, bool(lib.eqd_dock_is_simulator())
    return lib


def load_dock_library():
    """Load libequidock_dock.so built by equidock_public_amd/build.py.  Raises if it is missing."""
    if _dock is not None:
        return _dock
    if not os.path.exists(DOCK_LIB_PATH):
        raise _lib.EquidockHipError(f"{DOCK_LIB_PATH} is missing: build it with `python -m equidock_public_amd.build` "
                                    "(hipcc, gfx950).  There is no CPU fallback for batched clash removal.")
    return _bind(DOCK_LIB_PATH)


def load_dock_library_for_testing(path):
    """TESTS ONLY: bind an explicitly given build of the dock ABI (the x86 simulator build of csrc_dock/)."""
    return _bind(path)


def unload_dock_for_testing():
    global _dock, _dock_is_sim
    _dock, _dock_is_sim = None, False


def check(rc):
    if rc != 0:
        raise _lib.EquidockHipError(f"libequidock_dock error {rc}: {_dock.eqd_dock_last_error().decode()}")


def _require_device(t, what):
    if _dock_is_sim:
        if t.is_cuda:
            raise _lib.EquidockHipError(f"{what}: the host simulator only takes CPU tensors")
    elif not t.is_cuda:
        raise _lib.EquidockHipError(f"{what} is on {t.device}: batched docking inference runs only on an MI355X through "
                                    "libequidock_dock.so (no CPU fallback)")
    return t


def _stream(dev):
    return C.c_void_p(0) if _dock_is_sim else C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    if off[-1] > np.iinfo(np.int32).max:
        raise ValueError(f"{int(off[-1])} atoms do not fit int32 offsets: split the batch")
    return np.ascontiguousarray(off.astype(np.int32))


def remove_clashes_batch(ligand_atoms_list, receptor_atoms_list, sigma=8.0, surface_ct=8.0, loss_stop=0.5, max_it=2000,
                         check_every=50):
    """inference.remove_clashes for C complexes in one device loop.  ligand_atoms_list[c] [n_c, 3]: the docked ligand of
    complex c (all atoms, after apply_rigid); receptor_atoms_list[c] [m_c, 3].  `max_it`: an int or one per complex.
    Returns one dict per complex with the keys and meaning of remove_clashes (positions, euler, translation, iterations,
    loss).  The host reads the 4-byte completion counter every `check_every` iterations."""
    lib = load_dock_library()
    ligs, recs = list(ligand_atoms_list), list(receptor_atoms_list)
    if len(ligs) != len(recs):
        raise ValueError(f"{len(ligs)} ligands for {len(recs)} receptors")
    n = len(ligs)
    if n == 0:
        return []
    caps = [int(max_it)] * n if np.ndim(max_it) == 0 else [int(v) for v in max_it]
    if len(caps) != n:
        raise ValueError(f"{len(caps)} max_it values for {n} complexes")
    if int(check_every) < 1:
        raise ValueError(f"check_every = {check_every}")
    ligs = [_require_device(x.detach().to(torch.float32).reshape(-1, 3).contiguous(), f'ligand atoms {i}') for i, x in enumerate(ligs)]
    recs = [_require_device(x.detach().to(torch.float32).reshape(-1, 3).contiguous(), f'receptor atoms {i}') for i, x in enumerate(recs)]
    dev = ligs[0].device
    lig_off, rec_off = _offsets([x.shape[0] for x in ligs]), _offsets([x.shape[0] for x in recs])
    caps_np = np.ascontiguousarray(np.asarray(caps, dtype=np.int32))
    lo, ro = lig_off.ctypes.data_as(C.c_void_p), rec_off.ctypes.data_as(C.c_void_p)
    wsb = lib.eqd_dock_clash_workspace_bytes(n, lo, ro)
    if wsb == 0:
        check(2)
    lig_cat, rec_cat = torch.cat(ligs, 0), torch.cat(recs, 0)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    states = torch.empty(n * C.sizeof(INF.EqdClashState), dtype=torch.uint8, device=dev)
    n_done = torch.empty(1, dtype=torch.int32, device=dev)
    st = _stream(dev)
    with _lib.device_guard(dev):
        check(lib.eqd_dock_clash_init(n, lo, ro, caps_np.ctypes.data_as(C.c_void_p), _lib.ptr(states), _lib.ptr(n_done),
                                      _lib.ptr(ws), C.c_size_t(wsb), st))
        issued, bound = 0, max(max(caps), 0) + 1      # every complex has finished after max(max_it) + 1 iterations
        while True:
            n_iter = min(int(check_every), bound - issued)
            issued += n_iter
            check(lib.eqd_dock_clash_iterations(n_iter, n, lo, ro, _lib.ptr(lig_cat), _lib.ptr(rec_cat),
                                                C.c_float(sigma), C.c_float(surface_ct), C.c_float(loss_stop),
                                                _lib.ptr(states), _lib.ptr(n_done), _lib.ptr(ws), C.c_size_t(wsb), st))
            if int(n_done.cpu()[0]) >= n:          # the periodic look at the completion counter
                break
            if issued >= bound:
                raise _lib.EquidockHipError(f"clash removal: {int(n_done.cpu()[0])} of {n} complexes finished after "
                                            f"{issued} iterations (max_it {max(caps)})")
    host = (INF.EqdClashState * n).from_buffer_copy(states.cpu().numpy().tobytes())
    out = []
    for c in range(n):
        euler = np.asarray(host[c].euler[:], dtype=np.float32)
        trans = np.asarray(host[c].trans[:], dtype=np.float32)
        pos = INF.apply_rigid(INF.get_rot_mat(torch.from_numpy(euler)).to(dev), trans, ligs[c])
        out.append({'positions': pos, 'euler': euler, 'translation': trans, 'iterations': int(host[c].it),
                    'loss': float(host[c].loss)})
    return out


# ---- batched RMSD meter -----------------------------------------------------------------------------------------------
class MeterPlan:
    """Workspace of eqd_dock_meter_eval for one set of host offsets: created and initialised once (init copies the item
    table and waits for that copy), then `eval` only enqueues launches - it can be captured into a hipGraph."""

    def __init__(self, lig_off, rec_off, dev):
        lib = load_dock_library()
        self.lig_off = np.ascontiguousarray(np.asarray(lig_off, dtype=np.int32))
        self.rec_off = np.ascontiguousarray(np.asarray(rec_off, dtype=np.int32))
        if len(self.lig_off) != len(self.rec_off) or len(self.lig_off) < 2:
            raise ValueError(f"{len(self.lig_off)} ligand offsets for {len(self.rec_off)} receptor offsets")
        self.n, self.dev = len(self.lig_off) - 1, torch.device(dev)
        self._lo, self._ro = self.lig_off.ctypes.data_as(C.c_void_p), self.rec_off.ctypes.data_as(C.c_void_p)
        self.wsb = lib.eqd_dock_meter_workspace_bytes(self.n, self._lo, self._ro)
        if self.wsb == 0:
            check(2)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=self.dev)
        with _lib.device_guard(self.dev):
            check(lib.eqd_dock_meter_init(self.n, self._lo, self._ro, _lib.ptr(self.ws), C.c_size_t(self.wsb),
                                          _stream(self.dev)))

    def eval(self, lig_pred, rec_pred, lig_true, rec_true, out, cutoff=8.0, interface=True):
        """Enqueue the metric pass on the current stream: [sum n][3] fp32 contiguous inputs (rec_pred may be None: it is
        rec_true), out [C][8] fp64.  No synchronisation, no allocation, no copy."""
        with _lib.device_guard(self.dev):
            check(_dock.eqd_dock_meter_eval(self.n, self._lo, self._ro, _lib.ptr(lig_pred),
                                            _lib.ptr(rec_pred) if rec_pred is not None else C.c_void_p(0),
                                            _lib.ptr(lig_true), _lib.ptr(rec_true), C.c_double(float(cutoff)),
                                            int(bool(interface)), _lib.ptr(out), _lib.ptr(self.ws), C.c_size_t(self.wsb),
                                            _stream(self.dev)))
        return out


def _meter_rows(ts, what):
    return [_require_device(x.detach().to(torch.float32).reshape(-1, 3).contiguous(), f'{what} {i}') for i, x in enumerate(ts)]


def rmsd_metrics_batch(lig_pred_list, lig_true_list, rec_true_list, rec_pred_list=None, cutoff=8.0, interface=True):
    """inference.rmsd_metrics and inference.complex_and_interface_rmsd for C complexes in one device pass
    (eqd_dock_meter_*): per complex the ligand and receptor RMSD (no alignment), the complex RMSD after Kabsch
    superposition of all rows, and - with `interface` - the interface RMSD over the pairs of the ground truth closer than
    `cutoff` (NaN for a complex without such a pair) and their number.  `rec_pred_list` None: the receptor is its own
    prediction, as in src/train.py:137-140.  fp64 on the device from the fp32 rows; a complex's row is bit-identical
    alone, in any batch and from run to run.

    Returns a dict of device float64 tensors [C]: ligand_rmsd, receptor_rmsd, complex_rmsd, interface_rmsd,
    interface_pairs, flags (bit 0 / bit 1: the Kabsch of the complex / interface set took the reflection branch), and
    `metrics`, the raw [C][8] buffer.  Apart from the item-table copy of the workspace's init, the call does not
    synchronise and downloads nothing."""
    ligs_p, ligs_t, recs_t = list(lig_pred_list), list(lig_true_list), list(rec_true_list)
    recs_p = None if rec_pred_list is None else list(rec_pred_list)
    n = len(ligs_p)
    if not (n == len(ligs_t) == len(recs_t)) or (recs_p is not None and len(recs_p) != n):
        raise ValueError(f"{n} predicted ligands for {len(ligs_t)} true ligands, {len(recs_t)} true receptors and "
                         f"{'no' if recs_p is None else len(recs_p)} predicted receptors")
    if n == 0:
        raise ValueError("rmsd_metrics_batch: no complexes")
    ligs_p, ligs_t, recs_t = _meter_rows(ligs_p, 'predicted ligand'), _meter_rows(ligs_t, 'true ligand'), _meter_rows(recs_t, 'true receptor')
    if recs_p is not None:
        recs_p = _meter_rows(recs_p, 'predicted receptor')
    for c in range(n):
        if ligs_p[c].shape[0] != ligs_t[c].shape[0]:
            raise ValueError(f"complex {c}: {ligs_p[c].shape[0]} predicted ligand rows for {ligs_t[c].shape[0]} true ones")
        if recs_p is not None and recs_p[c].shape[0] != recs_t[c].shape[0]:
            raise ValueError(f"complex {c}: {recs_p[c].shape[0]} predicted receptor rows for {recs_t[c].shape[0]} true ones")
    dev = ligs_p[0].device
    plan = MeterPlan(_offsets([x.shape[0] for x in ligs_t]), _offsets([x.shape[0] for x in recs_t]), dev)
    out = torch.empty(n, METER_COLS, dtype=torch.float64, device=dev)
    plan.eval(torch.cat(ligs_p, 0), None if recs_p is None else torch.cat(recs_p, 0), torch.cat(ligs_t, 0),
              torch.cat(recs_t, 0), out, cutoff=cutoff, interface=interface)
    return {'ligand_rmsd': out[:, 0], 'receptor_rmsd': out[:, 1], 'complex_rmsd': out[:, 2], 'interface_rmsd': out[:, 3],
            'interface_pairs': out[:, 4], 'flags': out[:, 5], 'metrics': out}


class DeviceMeter:
    """inference.Meter_Unbound_Bound (src/utils/eval.py:12-77, same method names) for whole batches: `update_batch`
    appends the batch's metric rows on the device without synchronising, the summaries download the accumulated rows
    once.  `interface`: also evaluate the interface RMSD (summarize_interface)."""

    def __init__(self, cutoff=8.0, interface=False):
        self.cutoff, self.interface = float(cutoff), bool(interface)
        self._rows = []          # [C][8] device tensors

    def __len__(self):
        return sum(int(r.shape[0]) for r in self._rows)

    def update_batch(self, lig_pred_list, rec_pred_list, lig_true_list, rec_true_list):
        """One rmsd_metrics_batch over the lists (rec_pred_list may be None); returns the batch's complex RMSDs [C] on
        the device."""
        m = rmsd_metrics_batch(lig_pred_list, lig_true_list, rec_true_list, rec_pred_list, cutoff=self.cutoff,
                               interface=self.interface)
        self._rows.append(m['metrics'])
        return m['complex_rmsd']

    def update_rmsd(self, ligand_coors_pred, receptor_coors_pred, ligand_coors_true, receptor_coors_true):
        """The host meter's signature: a batch of one (returns the complex RMSD as a device scalar)."""
        return self.update_batch([ligand_coors_pred], [receptor_coors_pred], [ligand_coors_true], [receptor_coors_true])[0]

    def append_rows(self, rows):
        """Take a copy of a [C][8] metrics buffer the caller has filled (a device-to-device copy on the current stream)."""
        if rows.dim() != 2 or rows.shape[1] != METER_COLS or rows.dtype != torch.float64:
            raise ValueError(f"append_rows: expected a float64 [C][{METER_COLS}] buffer, got {rows.dtype} {tuple(rows.shape)}")
        self._rows.append(rows.detach().clone())

    def rows(self):
        """The accumulated [N][8] rows on the host (ONE download)."""
        if not self._rows:
            return np.zeros((0, METER_COLS), dtype=np.float64)
        return (self._rows[0] if len(self._rows) == 1 else torch.cat(self._rows, 0)).cpu().numpy()

    @staticmethod
    def _reduction(reduction_rmsd):
        if reduction_rmsd not in ('mean', 'median'):
            raise ValueError("Meter_Unbound_Bound: reduction_rmsd mis specified!")
        return np.mean if reduction_rmsd == 'mean' else np.median

    def summarize(self, reduction_rmsd='median'):
        f = self._reduction(reduction_rmsd)
        r = self.rows()
        return f(r[:, 0]), f(r[:, 1]), f(r[:, 2])

    def summarize_with_std(self, reduction_rmsd='median'):
        f = self._reduction(reduction_rmsd)
        arr = self.rows()[:, 2]
        return f(arr), np.std(arr)

    def summarize_interface(self, reduction_rmsd='median'):
        """(reduced interface RMSD, its std) over the complexes that have an interface."""
        f = self._reduction(reduction_rmsd)
        arr = self.rows()[:, 3]
        arr = arr[~np.isnan(arr)]
        if arr.size == 0:
            return float('nan'), float('nan')
        return f(arr), np.std(arr)


# ---- batched exact transport plans -----------------------------------------------------------------------------------
def emd_resident_enabled():
    """EQD_DOCK_EMD_RESIDENT=0 forces the general body of the device solver (cost read from global memory, flow in the
    workspace) for every problem; same plans either way."""
    return os.environ.get('EQD_DOCK_EMD_RESIDENT', '1') != '0'


class EmdPlan:
    """Workspace and status buffer of eqd_dock_emd_solve for one ragged batch of transport problems with uniform marginals
    (problem p: counts[p] sources, n_snk sinks): created and initialised once (init copies the offset table and waits for
    that copy), then `solve` only enqueues ONE launch - it can be captured into a hipGraph."""

    def __init__(self, counts, n_snk, dev):
        lib = load_dock_library()
        self.counts = [int(c) for c in counts]
        if not self.counts or min(self.counts) < 0:
            raise ValueError(f"EmdPlan: counts = {self.counts} (need >= 1 problem, no negative count)")
        self.n, self.K, self.dev = len(self.counts), int(n_snk), torch.device(dev)
        _require_device(torch.empty(0, device=self.dev), 'transport problems')
        self.off = _offsets(self.counts)
        self.rows = int(self.off[-1])
        self._off = self.off.ctypes.data_as(C.c_void_p)
        self.wsb = lib.eqd_dock_emd_workspace_bytes(self.n, self._off, self.K)
        if self.wsb == 0:
            check(2)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=self.dev)
        self.status = torch.zeros(self.n, dtype=torch.int32, device=self.dev)
        with _lib.device_guard(self.dev):
            check(lib.eqd_dock_emd_init(self.n, self._off, self.K, _lib.ptr(self.ws), C.c_size_t(self.wsb), _stream(self.dev)))

    def solve(self, cost, plan, resident=None):
        """Enqueue the solve on the current stream: cost, plan [sum(counts)][n_snk] fp32 contiguous, bit-identical to
        losses.emd_uniform_host's plans.  No synchronisation, no allocation, no copy; `status` is written by the launch."""
        for t, what in ((cost, 'cost'), (plan, 'plan')):
            _require_device(t, what)
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (self.rows, self.K):
                raise ValueError(f"EmdPlan.solve: {what} must be a contiguous float32 [{self.rows}, {self.K}] tensor, got "
                                 f"{t.dtype} {tuple(t.shape)}")
        resident = emd_resident_enabled() if resident is None else bool(resident)
        with _lib.device_guard(self.dev):
            check(_dock.eqd_dock_emd_solve(self.n, self._off, self.K, _lib.ptr(cost), _lib.ptr(plan), _lib.ptr(self.status),
                                           int(resident), _lib.ptr(self.ws), C.c_size_t(self.wsb), _stream(self.dev)))
        return plan

    def failed(self):
        """Indices of the problems of the latest solve whose status is non-zero (ONE download; it synchronises)."""
        return [int(i) for i in np.nonzero(self.status.cpu().numpy())[0]]


def emd_uniform_batch(cost, counts, resident=None):
    """losses.emd_uniform_host on the device: exact plans of a ragged batch of transport problems with uniform marginals.
    cost: device float32 [sum(counts), K].  Returns (plan [sum(counts), K] float32, status [len(counts)] int32) on the
    device, without synchronising beyond the workspace's init; a failed problem (status 1) has a NaN plan."""
    cost = _require_device(cost.detach().to(torch.float32).contiguous(), 'cost')
    if cost.dim() != 2 or int(sum(int(c) for c in counts)) != cost.shape[0]:
        raise ValueError("counts do not add up to the rows of cost")
    ep = EmdPlan(counts, cost.shape[1], cost.device)
    plan = torch.empty_like(cost)
    ep.solve(cost, plan, resident=resident)
    return plan, ep.status


# ---- batched docking quality: fnat, LRMSD, iRMSD(bb), DockQ, clashes ------------------------------------------------------
BACKBONE = ('N', 'CA', 'C', 'O')
QUALITY_KEYS = ('dockq', 'fnat', 'fnonnat', 'irmsd_backbone', 'lrmsd', 'native_contacts', 'model_contacts', 'shared_contacts',
                'interface_residues_ligand', 'interface_residues_receptor', 'interface_backbone_rows', 'clashes', 'flags',
                'pruned_pairs')


def quality_pruning_enabled():
    """EQD_DOCK_QUALITY_PRUNE=0 turns the centroid-and-radius pruning of the residue-pair search off (same results but
    for the count of pruned pairs)."""
    return os.environ.get('EQD_DOCK_QUALITY_PRUNE', '1') != '0'


def _is_hydrogen(name, element):
    el = element.strip().upper()
    if el:
        return el in ('H', 'D')
    return name.strip().lstrip('0123456789')[:1].upper() in ('H', 'D')


def _atom_rows(x):
    """(residue key, name, element, xyz) of every ATOM row of a PDB path or of a list of featurize.Residue"""
    rows = []
    if isinstance(x, (str, os.PathLike)):
        with open(x) as f:
            for line in f:
                if line.startswith('ATOM'):
                    rows.append(((line[21:22], line[22:26], line[26:27], line[17:20]), line[12:16].strip(),
                                 line[76:78] if len(line) >= 78 else '',
                                 (float(line[30:38]), float(line[38:46]), float(line[46:54]))))
    else:
        for r in x:
            key = (r.chain, r.number, '', r.resname)
            els = r.elements if len(r.elements) == len(r.atom_names) else [''] * len(r.atom_names)
            for name, el, xyz in zip(r.atom_names, els, r.coords):
                rows.append((key, name.strip(), el, xyz))
    return rows


def atom_table(x):
    """The heavy atoms of a PDB path or of a list of featurize.Residue, in file (list) order:
    (coordinates [n, 3] float32, index [n] int64 of those rows among ALL ATOM rows - the rows of inference.read_pdb_atoms /
    featurize.atoms_ragged -, residue offsets [n_res + 1] int32 into the n rows, backbone mask [n] uint8 (atoms named N,
    CA, C or O), atom names [n]).  A residue is a maximal run of consecutive ATOM rows that share chain, residue number,
    insertion code and residue name - file order, not the sorted grouping of featurize.read_pdb_residues; a run whose
    atoms are all hydrogens has no row and no residue."""
    rows = _atom_rows(x)
    index, names, coords, off, prev = [], [], [], [0], None
    for k, (key, name, el, xyz) in enumerate(rows):
        new_run = key != prev
        prev = key
        if new_run and len(index) > off[-1]:
            off.append(len(index))
        if _is_hydrogen(name, el):
            continue
        index.append(k)
        names.append(name)
        coords.append(xyz)
    if len(index) > off[-1]:
        off.append(len(index))
    names = np.asarray(names, dtype=str)
    return (np.ascontiguousarray(np.asarray(coords, dtype=np.float32).reshape(-1, 3)), np.asarray(index, dtype=np.int64),
            np.asarray(off, dtype=np.int32), np.isin(names, BACKBONE).astype(np.uint8), names)


def _residue_table(off, n_atoms, what):
    off = np.asarray(off)
    if off.ndim != 1 or len(off) < 2 or int(off[0]) != 0 or int(off[-1]) != n_atoms or (np.diff(off.astype(np.int64)) < 1).any():
        raise ValueError(f"{what}: residue offsets must start at 0, increase strictly and end at the {n_atoms} atom rows")
    return off.astype(np.int64)


class QualityPlan:
    """Workspace and tables of eqd_dock_quality_eval for one batch of complexes: the per-complex residue offsets (local:
    [n_res + 1] into the complex's own rows) and backbone masks ([n_atoms], non-zero = N, CA, C or O) go up in ONE copy,
    the workspace is created and initialised once (init copies the item table and waits for that copy); `eval` then only
    enqueues launches - it can be captured into a hipGraph."""

    def __init__(self, lig_res_offsets, rec_res_offsets, lig_backbone, rec_backbone, dev):
        lib = load_dock_library()
        n = len(lig_res_offsets)
        if n == 0 or not (n == len(rec_res_offsets) == len(lig_backbone) == len(rec_backbone)):
            raise ValueError(f"{n} ligand residue tables for {len(rec_res_offsets)} receptor residue tables, "
                             f"{len(lig_backbone)} ligand and {len(rec_backbone)} receptor backbone masks")
        lbb = [np.asarray(m).reshape(-1) != 0 for m in lig_backbone]
        rbb = [np.asarray(m).reshape(-1) != 0 for m in rec_backbone]
        lro = [_residue_table(o, len(m), f'complex {c}: ligand') for c, (o, m) in enumerate(zip(lig_res_offsets, lbb))]
        rro = [_residue_table(o, len(m), f'complex {c}: receptor') for c, (o, m) in enumerate(zip(rec_res_offsets, rbb))]
        self.n, self.dev = n, torch.device(dev)
        self.lig_atom_off, self.rec_atom_off = _offsets([len(m) for m in lbb]), _offsets([len(m) for m in rbb])
        self.lig_res_off, self.rec_res_off = _offsets([len(o) - 1 for o in lro]), _offsets([len(o) - 1 for o in rro])
        self._off = tuple(a.ctypes.data_as(C.c_void_p) for a in (self.lig_atom_off, self.rec_atom_off, self.lig_res_off,
                                                                  self.rec_res_off))
        Al, Ar, Rl, Rr = (int(a[-1]) for a in (self.lig_atom_off, self.rec_atom_off, self.lig_res_off, self.rec_res_off))
        # one staging buffer, one upload: int32 first rows of the ligand | of the receptor residues, uint8 masks
        host = _staging(4 * (Rl + Rr + 2) + Al + Ar, torch.uint8, self.dev)
        h = host.numpy()
        first = h[:4 * (Rl + Rr + 2)].view(np.int32)
        first[:Rl + 1] = np.concatenate([o[:-1] + int(a) for o, a in zip(lro, self.lig_atom_off)] + [[Al]])
        first[Rl + 1:] = np.concatenate([o[:-1] + int(a) for o, a in zip(rro, self.rec_atom_off)] + [[Ar]])
        h[4 * (Rl + Rr + 2):] = np.concatenate(lbb + rbb)
        self.tables = host.to(self.dev, non_blocking=True)
        ints = self.tables[:4 * (Rl + Rr + 2)].view(torch.int32)
        self.lig_first, self.rec_first = ints[:Rl + 1], ints[Rl + 1:]
        self.lig_bb, self.rec_bb = self.tables[4 * (Rl + Rr + 2):4 * (Rl + Rr + 2) + Al], self.tables[4 * (Rl + Rr + 2) + Al:]
        self.residue_pairs = int(sum((len(a) - 1) * (len(b) - 1) for a, b in zip(lro, rro)))
        self.wsb = lib.eqd_dock_quality_workspace_bytes(n, *self._off)
        if self.wsb == 0:
            check(2)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=self.dev)
        with _lib.device_guard(self.dev):
            check(lib.eqd_dock_quality_init(n, *self._off, _lib.ptr(self.ws), C.c_size_t(self.wsb), _stream(self.dev)))

    def eval(self, lig_pred, rec_pred, lig_true, rec_true, out, contact_cutoff=5.0, interface_cutoff=10.0, clash_cutoff=3.0,
             prune=None):
        """Enqueue the quality pass on the current stream: [sum n][3] fp32 contiguous inputs (rec_pred may be None: it is
        rec_true), out [C][16] fp64.  No synchronisation, no allocation, no copy."""
        prune = quality_pruning_enabled() if prune is None else bool(prune)
        with _lib.device_guard(self.dev):
            check(_dock.eqd_dock_quality_eval(self.n, *self._off, _lib.ptr(lig_pred),
                                              _lib.ptr(rec_pred) if rec_pred is not None else C.c_void_p(0),
                                              _lib.ptr(lig_true), _lib.ptr(rec_true), _lib.ptr(self.lig_first),
                                              _lib.ptr(self.rec_first), _lib.ptr(self.lig_bb), _lib.ptr(self.rec_bb),
                                              C.c_double(float(contact_cutoff)), C.c_double(float(interface_cutoff)),
                                              C.c_double(float(clash_cutoff)), int(prune), _lib.ptr(out), _lib.ptr(self.ws),
                                              C.c_size_t(self.wsb), _stream(self.dev)))
        return out


def pose_quality_batch(lig_pred_list, lig_true_list, rec_true_list, lig_res_offsets=None, rec_res_offsets=None,
                       lig_backbone=None, rec_backbone=None, rec_pred_list=None, contact_cutoff=5.0, interface_cutoff=10.0,
                       clash_cutoff=3.0, plan=None):
    """fnat, LRMSD, backbone iRMSD, DockQ (Basu & Wallner 2016) and the steric clashes of C docked complexes in one device
    pass over every heavy atom (eqd_dock_quality_*; the definitions are in include/equidock_dock.h).  The lists hold device
    tensors [n_c, 3] of heavy atoms, the model's rows corresponding one to one to the native's; `rec_pred_list` None: the
    model's receptor is the native's.  Per complex (host arrays, as `atom_table` returns them): the residue offsets
    [n_res + 1] into its own rows and the backbone mask [n_c] of each side - or a `plan` (QualityPlan) that already holds
    them, so that repeated evaluation of the same complexes reuses tables and workspace.  fp64 on the device from the
    fp32 rows; a complex's row is bit-identical alone, in any batch and from run to run.

    Returns a dict of device float64 tensors [C] (QUALITY_KEYS: dockq, fnat, fnonnat, irmsd_backbone, lrmsd,
    native_contacts, model_contacts, shared_contacts, interface_residues_ligand / _receptor, interface_backbone_rows,
    clashes, flags - bit 0 / bit 1: the Kabsch of the interface / receptor backbone set took the reflection branch -,
    pruned_pairs), `quality`, the raw [C][16] buffer, and `plan`.  One upload of the small tables (when no plan is
    given), one launch sequence; apart from the item-table copy of the workspace's init the call does not synchronise and
    downloads nothing."""
    ligs_p, ligs_t, recs_t = list(lig_pred_list), list(lig_true_list), list(rec_true_list)
    recs_p = None if rec_pred_list is None else list(rec_pred_list)
    n = len(ligs_p)
    if not (n == len(ligs_t) == len(recs_t)) or (recs_p is not None and len(recs_p) != n):
        raise ValueError(f"{n} predicted ligands for {len(ligs_t)} true ligands, {len(recs_t)} true receptors and "
                         f"{'no' if recs_p is None else len(recs_p)} predicted receptors")
    if n == 0:
        raise ValueError("pose_quality_batch: no complexes")
    ligs_p, ligs_t, recs_t = _meter_rows(ligs_p, 'predicted ligand'), _meter_rows(ligs_t, 'true ligand'), _meter_rows(recs_t, 'true receptor')
    if recs_p is not None:
        recs_p = _meter_rows(recs_p, 'predicted receptor')
    for c in range(n):
        if ligs_p[c].shape[0] != ligs_t[c].shape[0]:
            raise ValueError(f"complex {c}: {ligs_p[c].shape[0]} predicted ligand rows for {ligs_t[c].shape[0]} true ones")
        if recs_p is not None and recs_p[c].shape[0] != recs_t[c].shape[0]:
            raise ValueError(f"complex {c}: {recs_p[c].shape[0]} predicted receptor rows for {recs_t[c].shape[0]} true ones")
    dev = ligs_p[0].device
    if plan is None:
        if lig_res_offsets is None or rec_res_offsets is None or lig_backbone is None or rec_backbone is None:
            raise ValueError("pose_quality_batch: residue offsets and backbone masks of both sides (or a plan) are needed")
        plan = QualityPlan(list(lig_res_offsets), list(rec_res_offsets), list(lig_backbone), list(rec_backbone), dev)
    if plan.n != n:
        raise ValueError(f"the plan holds {plan.n} complexes, the lists {n}")
    for c in range(n):
        nl, nr = int(plan.lig_atom_off[c + 1] - plan.lig_atom_off[c]), int(plan.rec_atom_off[c + 1] - plan.rec_atom_off[c])
        if ligs_t[c].shape[0] != nl or recs_t[c].shape[0] != nr:
            raise ValueError(f"complex {c}: {ligs_t[c].shape[0]} ligand and {recs_t[c].shape[0]} receptor rows for tables of "
                             f"{nl} and {nr} atoms")
    out = torch.empty(n, QUALITY_COLS, dtype=torch.float64, device=dev)
    plan.eval(torch.cat(ligs_p, 0), None if recs_p is None else torch.cat(recs_p, 0), torch.cat(ligs_t, 0),
              torch.cat(recs_t, 0), out, contact_cutoff=contact_cutoff, interface_cutoff=interface_cutoff,
              clash_cutoff=clash_cutoff)
    res = {k: out[:, i] for i, k in enumerate(QUALITY_KEYS)}
    res.update(quality=out, plan=plan)
    return res


# ---- batched solvent-accessible surface: SASA, buried surface area, buried atoms and residues ------------------------
SURFACE_KEYS = ('sasa_ligand', 'sasa_receptor', 'sasa_complex', 'bsa', 'bsa_ligand', 'bsa_receptor', 'buried_atoms_ligand',
                'buried_atoms_receptor', 'buried_residues_ligand', 'buried_residues_receptor', 'points_alone',
                'points_complex')
ATOM_RADII = {'C': 1.70, 'N': 1.55, 'O': 1.52, 'S': 1.80}
DEFAULT_RADIUS = 1.80


def surface_all_partners():
    """EQD_DOCK_SASA_ALL_PARTNERS=1 sends every atom of the surface pass down the path that walks all atoms of its complex
    instead of its neighbour list (the path of an atom whose list overflows); same results, bit for bit."""
    return os.environ.get('EQD_DOCK_SASA_ALL_PARTNERS', '0') == '1'


def sphere_points(n):
    """n unit vectors [n, 3] float64 on a golden-section spiral: z_k = 1 - (2k + 1) / n, rho = sqrt(1 - z_k^2),
    phi = k * pi * (3 - sqrt(5)), rows (rho cos phi, rho sin phi, z_k)."""
    n = int(n)
    if n < 1 or n > SASA_MAX_POINTS:
        raise ValueError(f"sphere_points: n = {n} (need 1..{SASA_MAX_POINTS})")
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    rho = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.ascontiguousarray(np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1))


def atom_radii(x):
    """float32 radii [n] of the rows of atom_table(x): C 1.70, N 1.55, O 1.52, S 1.80, anything else 1.80, by the element
    column when it is present, otherwise by the first letter of the atom name after leading digits."""
    out = []
    for _, name, el, _ in _atom_rows(x):
        if _is_hydrogen(name, el):
            continue
        sym = el.strip().upper() or name.strip().lstrip('0123456789')[:1].upper()
        out.append(ATOM_RADII.get(sym, DEFAULT_RADIUS))
    return np.asarray(out, dtype=np.float32)


def _radii_table(r, what):
    r = np.ascontiguousarray(np.asarray(r, dtype=np.float32).reshape(-1))
    if not (np.isfinite(r).all() and (r > 0).all()):
        raise ValueError(f"{what}: radii must be finite and > 0")
    return r


class SurfacePlan:
    """Workspace and tables of eqd_dock_sasa_eval for one batch of complexes: the sphere table, the per-complex residue
    offsets (local: [n_res + 1] into the complex's own rows) and the radii ([n_atoms] float32, finite and > 0) go up in ONE
    copy, the workspace is created and initialised once (init copies the item table and waits for that copy); `eval` then
    only enqueues launches - it can be captured into a hipGraph."""

    def __init__(self, lig_res_offsets, rec_res_offsets, lig_radii, rec_radii, dev, n_points=96):
        lib = load_dock_library()
        n = len(lig_res_offsets)
        if n == 0 or not (n == len(rec_res_offsets) == len(lig_radii) == len(rec_radii)):
            raise ValueError(f"{n} ligand residue tables for {len(rec_res_offsets)} receptor residue tables, "
                             f"{len(lig_radii)} ligand and {len(rec_radii)} receptor radius tables")
        lr = [_radii_table(r, f'complex {c}: ligand') for c, r in enumerate(lig_radii)]
        rr = [_radii_table(r, f'complex {c}: receptor') for c, r in enumerate(rec_radii)]
        lro = [_residue_table(o, len(r), f'complex {c}: ligand') for c, (o, r) in enumerate(zip(lig_res_offsets, lr))]
        rro = [_residue_table(o, len(r), f'complex {c}: receptor') for c, (o, r) in enumerate(zip(rec_res_offsets, rr))]
        self.n, self.dev, self.n_points = n, torch.device(dev), int(n_points)
        _require_device(torch.empty(0, device=self.dev), 'surface inputs')
        sphere = sphere_points(self.n_points)
        self.lig_atom_off, self.rec_atom_off = _offsets([len(r) for r in lr]), _offsets([len(r) for r in rr])
        self.lig_res_off, self.rec_res_off = _offsets([len(o) - 1 for o in lro]), _offsets([len(o) - 1 for o in rro])
        self._off = tuple(a.ctypes.data_as(C.c_void_p) for a in (self.lig_atom_off, self.rec_atom_off, self.lig_res_off,
                                                                  self.rec_res_off))
        Al, Ar, Rl, Rr = (int(a[-1]) for a in (self.lig_atom_off, self.rec_atom_off, self.lig_res_off, self.rec_res_off))
        self.sizes = (Al, Ar, Rl, Rr)
        # one staging buffer, one upload: fp64 sphere table | int32 first rows of the ligand, of the receptor residues |
        # fp32 radii of the ligand, of the receptor atoms
        nb_s, nb_f = 24 * self.n_points, 4 * (Rl + Rr + 2)
        host = _staging(nb_s + nb_f + 4 * (Al + Ar), torch.uint8, self.dev)
        h = host.numpy()
        h[:nb_s].view(np.float64)[:] = sphere.reshape(-1)
        first = h[nb_s:nb_s + nb_f].view(np.int32)
        first[:Rl + 1] = np.concatenate([o[:-1] + int(a) for o, a in zip(lro, self.lig_atom_off)] + [[Al]])
        first[Rl + 1:] = np.concatenate([o[:-1] + int(a) for o, a in zip(rro, self.rec_atom_off)] + [[Ar]])
        h[nb_s + nb_f:].view(np.float32)[:] = np.concatenate(lr + rr)
        self.tables = host.to(self.dev, non_blocking=True)
        self.sphere = self.tables[:nb_s].view(torch.float64).view(self.n_points, 3)
        ints = self.tables[nb_s:nb_s + nb_f].view(torch.int32)
        self.lig_first, self.rec_first = ints[:Rl + 1], ints[Rl + 1:]
        rad = self.tables[nb_s + nb_f:].view(torch.float32)
        self.lig_radii, self.rec_radii = rad[:Al], rad[Al:]
        self.atom_pairs = int(sum((a + b) * (a + b - 1) for a, b in zip(np.diff(self.lig_atom_off).astype(np.int64),
                                                                         np.diff(self.rec_atom_off).astype(np.int64))))
        self.wsb = lib.eqd_dock_sasa_workspace_bytes(n, *self._off, self.n_points)
        if self.wsb == 0:
            check(2)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=self.dev)
        with _lib.device_guard(self.dev):
            check(lib.eqd_dock_sasa_init(n, *self._off, self.n_points, _lib.ptr(self.ws), C.c_size_t(self.wsb),
                                         _stream(self.dev)))

    def outputs(self):
        """Freshly allocated output buffers of one eval: (points [A_l + A_r][2] int32, residue areas [R_l + R_r][2] fp64,
        rows [C][12] fp64); the ligand's rows come first in the first two."""
        Al, Ar, Rl, Rr = self.sizes
        return (torch.empty(Al + Ar, 2, dtype=torch.int32, device=self.dev),
                torch.empty(Rl + Rr, 2, dtype=torch.float64, device=self.dev),
                torch.empty(self.n, SASA_COLS, dtype=torch.float64, device=self.dev))

    def eval(self, lig, rec, points, res_area, rows, probe=1.4, all_partners=None):
        """Enqueue the surface pass on the current stream: lig [A_l][3], rec [A_r][3] fp32 contiguous, the buffers of
        `outputs()`.  No synchronisation, no allocation, no copy."""
        Al, Ar, Rl, Rr = self.sizes
        all_partners = surface_all_partners() if all_partners is None else bool(all_partners)
        with _lib.device_guard(self.dev):
            check(_dock.eqd_dock_sasa_eval(self.n, *self._off, _lib.ptr(lig), _lib.ptr(rec), _lib.ptr(self.lig_radii),
                                           _lib.ptr(self.rec_radii), _lib.ptr(self.lig_first), _lib.ptr(self.rec_first),
                                           _lib.ptr(self.sphere), self.n_points, C.c_double(float(probe)),
                                           int(all_partners), _lib.ptr(points[:Al]), _lib.ptr(points[Al:]),
                                           _lib.ptr(res_area[:Rl]), _lib.ptr(res_area[Rl:]), _lib.ptr(rows),
                                           _lib.ptr(self.ws), C.c_size_t(self.wsb), _stream(self.dev)))
        return rows


def surface_area_batch(lig_list, rec_list, lig_radii=None, rec_radii=None, lig_res_offsets=None, rec_res_offsets=None,
                       probe=1.4, n_points=96, plan=None):
    """Solvent-accessible surface of C complexes in one device pass over every heavy atom (eqd_dock_sasa_*; the
    definitions are in include/equidock_dock.h): Shrake-Rupley with `n_points` golden-spiral points per atom and a probe
    of `probe` Angstrom.  It needs no native structure.  The lists hold device tensors [n_c, 3] of heavy atoms; per complex
    (host arrays, as `atom_radii` / `atom_table` return them) the radii [n_c] (finite, > 0) and the residue offsets
    [n_res + 1] into its own rows of each side - or a `plan` (SurfacePlan) that already holds them, so that repeated
    evaluation of the same complexes reuses tables and workspace.  fp64 on the device from the fp32 rows; a complex's
    results are bit-identical alone, in any batch and from run to run.

    Returns a dict of device tensors: SURFACE_KEYS (float64 [C]: sasa_ligand, sasa_receptor, sasa_complex, bsa, bsa_ligand,
    bsa_receptor, buried_atoms_ligand / _receptor, buried_residues_ligand / _receptor, points_alone, points_complex),
    `rows`, the raw [C][12] buffer, `lig_points` / `rec_points` (int32 [A][2]: exposed points alone, in complex),
    `lig_res_area` / `rec_res_area` (float64 [R][2]) and `plan`.  One upload of the small tables (when no plan is given),
    one launch sequence; apart from the item-table copy of the workspace's init the call does not synchronise and
    downloads nothing."""
    ligs, recs = list(lig_list), list(rec_list)
    n = len(ligs)
    if n != len(recs):
        raise ValueError(f"{n} ligands for {len(recs)} receptors")
    if n == 0:
        raise ValueError("surface_area_batch: no complexes")
    ligs, recs = _meter_rows(ligs, 'ligand'), _meter_rows(recs, 'receptor')
    dev = ligs[0].device
    if plan is None:
        if lig_radii is None or rec_radii is None or lig_res_offsets is None or rec_res_offsets is None:
            raise ValueError("surface_area_batch: radii and residue offsets of both sides (or a plan) are needed")
        plan = SurfacePlan(list(lig_res_offsets), list(rec_res_offsets), list(lig_radii), list(rec_radii), dev,
                           n_points=n_points)
    if plan.n != n:
        raise ValueError(f"the plan holds {plan.n} complexes, the lists {n}")
    for c in range(n):
        nl, nr = int(plan.lig_atom_off[c + 1] - plan.lig_atom_off[c]), int(plan.rec_atom_off[c + 1] - plan.rec_atom_off[c])
        if ligs[c].shape[0] != nl or recs[c].shape[0] != nr:
            raise ValueError(f"complex {c}: {ligs[c].shape[0]} ligand and {recs[c].shape[0]} receptor rows for tables of "
                             f"{nl} and {nr} atoms")
    points, res_area, rows = plan.outputs()
    plan.eval(torch.cat(ligs, 0), torch.cat(recs, 0), points, res_area, rows, probe=probe)
    Al, Rl = plan.sizes[0], plan.sizes[2]
    res = {k: rows[:, i] for i, k in enumerate(SURFACE_KEYS)}
    res.update(rows=rows, lig_points=points[:Al], rec_points=points[Al:], lig_res_area=res_area[:Rl],
               rec_res_area=res_area[Rl:], plan=plan)
    return res


# ---- batched lDDT and interface lDDT --------------------------------------------------------------------------------
LDDT_KEYS = ('lddt', 'ilddt', 'lddt_ligand', 'lddt_receptor', 'pairs', 'interface_pairs', 'preserved_0', 'preserved_1',
             'preserved_2', 'preserved_3', 'interface_preserved_0', 'interface_preserved_1', 'interface_preserved_2',
             'interface_preserved_3', 'skipped_block_pairs')
LDDT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def lddt_pruning_enabled():
    """EQD_DOCK_LDDT_PRUNE=0 turns the centroid-and-radius bound on block pairs of the lDDT pass off (same results but for
    the count of skipped block pairs)."""
    return os.environ.get('EQD_DOCK_LDDT_PRUNE', '1') != '0'


class LddtPlan:
    """Workspace and tables of eqd_dock_lddt_eval for one batch of complexes: the per-complex residue offsets (local:
    [n_res + 1] into the complex's own rows) go up in ONE copy, the workspace is created and initialised once (init copies
    the item table and waits for that copy); `eval` then only enqueues launches - it can be captured into a hipGraph."""

    def __init__(self, lig_res_offsets, rec_res_offsets, dev):
        lib = load_dock_library()
        n = len(lig_res_offsets)
        if n == 0 or n != len(rec_res_offsets):
            raise ValueError(f"{n} ligand residue tables for {len(rec_res_offsets)} receptor residue tables")
        # (a table's last entry is its side's atom count; lddt_batch compares it with the rows it is given)
        lro = [_residue_table(o, int(np.asarray(o).reshape(-1)[-1:].sum()), f'complex {c}: ligand')
               for c, o in enumerate(lig_res_offsets)]
        rro = [_residue_table(o, int(np.asarray(o).reshape(-1)[-1:].sum()), f'complex {c}: receptor')
               for c, o in enumerate(rec_res_offsets)]
        self.n, self.dev = n, torch.device(dev)
        _require_device(torch.empty(0, device=self.dev), 'lDDT inputs')
        self.lig_atom_off, self.rec_atom_off = _offsets([int(o[-1]) for o in lro]), _offsets([int(o[-1]) for o in rro])
        self.lig_res_off, self.rec_res_off = _offsets([len(o) - 1 for o in lro]), _offsets([len(o) - 1 for o in rro])
        self._off = tuple(a.ctypes.data_as(C.c_void_p) for a in (self.lig_atom_off, self.rec_atom_off, self.lig_res_off,
                                                                  self.rec_res_off))
        Al, Ar, Rl, Rr = (int(a[-1]) for a in (self.lig_atom_off, self.rec_atom_off, self.lig_res_off, self.rec_res_off))
        self.sizes = (Al, Ar, Rl, Rr)
        # one staging buffer, one upload: int32 first rows of the ligand | of the receptor residues
        host = _staging(Rl + Rr + 2, torch.int32, self.dev)
        first = host.numpy()
        first[:Rl + 1] = np.concatenate([o[:-1] + int(a) for o, a in zip(lro, self.lig_atom_off)] + [[Al]])
        first[Rl + 1:] = np.concatenate([o[:-1] + int(a) for o, a in zip(rro, self.rec_atom_off)] + [[Ar]])
        self.tables = host.to(self.dev, non_blocking=True)
        self.lig_first, self.rec_first = self.tables[:Rl + 1], self.tables[Rl + 1:]
        n_at = np.diff(self.lig_atom_off).astype(np.int64) + np.diff(self.rec_atom_off).astype(np.int64)
        self.atom_pairs = int((n_at * (n_at - 1)).sum())
        self.wsb = lib.eqd_dock_lddt_workspace_bytes(n, *self._off)
        if self.wsb == 0:
            check(2)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=self.dev)
        with _lib.device_guard(self.dev):
            check(lib.eqd_dock_lddt_init(n, *self._off, _lib.ptr(self.ws), C.c_size_t(self.wsb), _stream(self.dev)))

    def outputs(self):
        """Freshly allocated output buffers of one eval: (counts [A_l + A_r][10] int32, residue scores [R_l + R_r][2] fp64,
        rows [C][16] fp64); the ligand's rows come first in the first two."""
        Al, Ar, Rl, Rr = self.sizes
        return (torch.empty(Al + Ar, 10, dtype=torch.int32, device=self.dev),
                torch.empty(Rl + Rr, 2, dtype=torch.float64, device=self.dev),
                torch.empty(self.n, LDDT_COLS, dtype=torch.float64, device=self.dev))

    def eval(self, lig_pred, rec_pred, lig_true, rec_true, counts, res_lddt, rows, inclusion_radius=15.0,
             thresholds=LDDT_THRESHOLDS, prune=None):
        """Enqueue the lDDT pass on the current stream: [sum n][3] fp32 contiguous inputs (rec_pred may be None: it is
        rec_true), the buffers of `outputs()`.  No synchronisation, no allocation, no copy."""
        Al, Ar, Rl, Rr = self.sizes
        prune = lddt_pruning_enabled() if prune is None else bool(prune)
        thr = [float(t) for t in thresholds]
        if len(thr) != 4:
            raise ValueError(f"{len(thr)} thresholds (need 4)")
        with _lib.device_guard(self.dev):
            check(_dock.eqd_dock_lddt_eval(self.n, *self._off, _lib.ptr(lig_pred),
                                           _lib.ptr(rec_pred) if rec_pred is not None else C.c_void_p(0),
                                           _lib.ptr(lig_true), _lib.ptr(rec_true), _lib.ptr(self.lig_first),
                                           _lib.ptr(self.rec_first), C.c_double(float(inclusion_radius)),
                                           (C.c_double * 4)(*thr), int(prune), _lib.ptr(counts[:Al]), _lib.ptr(counts[Al:]),
                                           _lib.ptr(res_lddt[:Rl]), _lib.ptr(res_lddt[Rl:]), _lib.ptr(rows),
                                           _lib.ptr(self.ws), C.c_size_t(self.wsb), _stream(self.dev)))
        return rows


def lddt_batch(lig_pred_list, lig_true_list, rec_true_list, lig_res_offsets=None, rec_res_offsets=None, rec_pred_list=None,
               inclusion_radius=15.0, thresholds=LDDT_THRESHOLDS, plan=None):
    """lDDT (Mariani et al. 2013) and interface lDDT of C docked complexes in one device pass over every heavy atom
    (eqd_dock_lddt_*; the definitions are in include/equidock_dock.h): the fraction of the native's atom pairs in
    different residues and closer than `inclusion_radius` whose distance the model keeps within each of the four
    `thresholds`, averaged over them - over all pairs and over the inter-chain pairs alone.  No superposition is involved.
    The lists hold device tensors [n_c, 3] of heavy atoms, the model's rows corresponding one to one to the native's;
    `rec_pred_list` None: the model's receptor is the native's.  Per complex (host arrays, as `atom_table` returns them)
    the residue offsets [n_res + 1] into its own rows of each side - or a `plan` (LddtPlan) that already holds them, so
    that repeated evaluation of the same complexes reuses tables and workspace.  fp64 on the device from the fp32 rows;
    every result is a count or a quotient of counts: a complex's results are bit-identical alone, in any batch and from run
    to run.

    Returns a dict of device tensors: LDDT_KEYS (float64 [C]: lddt, ilddt, lddt_ligand, lddt_receptor - NaN without an
    included pair -, pairs, interface_pairs, preserved_0..3, interface_preserved_0..3, skipped_block_pairs), `rows`, the
    raw [C][16] buffer, `lig_counts` / `rec_counts` (int32 [A][10]: n_all, p_all[4], n_inter, p_inter[4]), `lig_res_lddt` /
    `rec_res_lddt` (float64 [R][2]: residue lDDT, residue interface lDDT) and `plan`.  One upload of the small tables
    (when no plan is given), one launch sequence; apart from the item-table copy of the workspace's init the call does not
    synchronise and downloads nothing."""
    ligs_p, ligs_t, recs_t = list(lig_pred_list), list(lig_true_list), list(rec_true_list)
    recs_p = None if rec_pred_list is None else list(rec_pred_list)
    n = len(ligs_p)
    if not (n == len(ligs_t) == len(recs_t)) or (recs_p is not None and len(recs_p) != n):
        raise ValueError(f"{n} predicted ligands for {len(ligs_t)} true ligands, {len(recs_t)} true receptors and "
                         f"{'no' if recs_p is None else len(recs_p)} predicted receptors")
    if n == 0:
        raise ValueError("lddt_batch: no complexes")
    ligs_p, ligs_t, recs_t = _meter_rows(ligs_p, 'predicted ligand'), _meter_rows(ligs_t, 'true ligand'), _meter_rows(recs_t, 'true receptor')
    if recs_p is not None:
        recs_p = _meter_rows(recs_p, 'predicted receptor')
    for c in range(n):
        if ligs_p[c].shape[0] != ligs_t[c].shape[0]:
            raise ValueError(f"complex {c}: {ligs_p[c].shape[0]} predicted ligand rows for {ligs_t[c].shape[0]} true ones")
        if recs_p is not None and recs_p[c].shape[0] != recs_t[c].shape[0]:
            raise ValueError(f"complex {c}: {recs_p[c].shape[0]} predicted receptor rows for {recs_t[c].shape[0]} true ones")
    dev = ligs_p[0].device
    if plan is None:
        if lig_res_offsets is None or rec_res_offsets is None:
            raise ValueError("lddt_batch: residue offsets of both sides (or a plan) are needed")
        plan = LddtPlan(list(lig_res_offsets), list(rec_res_offsets), dev)
    if plan.n != n:
        raise ValueError(f"the plan holds {plan.n} complexes, the lists {n}")
    for c in range(n):
        nl, nr = int(plan.lig_atom_off[c + 1] - plan.lig_atom_off[c]), int(plan.rec_atom_off[c + 1] - plan.rec_atom_off[c])
        if ligs_t[c].shape[0] != nl or recs_t[c].shape[0] != nr:
            raise ValueError(f"complex {c}: {ligs_t[c].shape[0]} ligand and {recs_t[c].shape[0]} receptor rows for tables of "
                             f"{nl} and {nr} atoms")
    counts, res_lddt, rows = plan.outputs()
    plan.eval(torch.cat(ligs_p, 0), None if recs_p is None else torch.cat(recs_p, 0), torch.cat(ligs_t, 0),
              torch.cat(recs_t, 0), counts, res_lddt, rows, inclusion_radius=inclusion_radius, thresholds=thresholds)
    Al, Rl = plan.sizes[0], plan.sizes[2]
    res = {k: rows[:, i] for i, k in enumerate(LDDT_KEYS)}
    res.update(rows=rows, lig_counts=counts[:Al], rec_counts=counts[Al:], lig_res_lddt=res_lddt[:Rl],
               rec_res_lddt=res_lddt[Rl:], plan=plan)
    return res


# ---- batched residue depth ------------------------------------------------------------------------------------------
DEPTH_KEYS = ('depth_ligand', 'depth_receptor', 'depth_complex', 'max_depth_ligand', 'max_depth_receptor',
              'max_depth_complex', 'depth_gain_ligand', 'depth_gain_receptor', 'deepened_atoms_ligand',
              'deepened_atoms_receptor', 'deepened_residues_ligand', 'deepened_residues_receptor', 'vertices_alone',
              'vertices_complex', 'skipped_groups', 'flags')


def depth_pruning_enabled():
    """EQD_DOCK_DEPTH_PRUNE=0 turns the centre-and-reach bound on vertex groups of the depth pass off (same results but
    for the count of skipped groups)."""
    return os.environ.get('EQD_DOCK_DEPTH_PRUNE', '1') != '0'


def _ca_rows(names, off, n_atoms, what):
    """local row of the first atom named CA of every residue of a side, -1 where there is none (`names` None: all -1)"""
    ca = np.full(len(off) - 1, -1, dtype=np.int64)
    if names is None:
        return ca
    names = np.asarray(names, dtype=str).reshape(-1)
    if len(names) != n_atoms:
        raise ValueError(f"{what}: {len(names)} atom names for {n_atoms} atom rows")
    rows = np.nonzero(np.char.strip(names) == 'CA')[0]
    res = np.searchsorted(off, rows, side='right') - 1
    ca[res[::-1]] = rows[::-1]                                  # (the first CA row of a residue wins)
    return ca


class DepthPlan:
    """Workspace and tables of eqd_dock_depth_eval for one batch of complexes: the sphere table, the per-complex residue
    offsets (local: [n_res + 1] into the complex's own rows), the rows of the residues' CA atoms (from `lig_names` /
    `rec_names`, the atom names [n_atoms] of each complex as `atom_table` returns them; without them every CA row is -1)
    and the radii ([n_atoms] float32, finite and > 0) go up in ONE copy, the workspace is created and initialised once
    (init copies the tile table and waits for that copy); `eval` then only enqueues launches - it can be captured into a
    hipGraph."""

    def __init__(self, lig_res_offsets, rec_res_offsets, lig_radii, rec_radii, dev, n_points=96, lig_names=None,
                 rec_names=None):
        lib = load_dock_library()
        n = len(lig_res_offsets)
        if n == 0 or not (n == len(rec_res_offsets) == len(lig_radii) == len(rec_radii)):
            raise ValueError(f"{n} ligand residue tables for {len(rec_res_offsets)} receptor residue tables, "
                             f"{len(lig_radii)} ligand and {len(rec_radii)} receptor radius tables")
        for nm, what in ((lig_names, 'ligand'), (rec_names, 'receptor')):
            if nm is not None and len(nm) != n:
                raise ValueError(f"{len(nm)} {what} name tables for {n} complexes")
        lr = [_radii_table(r, f'complex {c}: ligand') for c, r in enumerate(lig_radii)]
        rr = [_radii_table(r, f'complex {c}: receptor') for c, r in enumerate(rec_radii)]
        lro = [_residue_table(o, len(r), f'complex {c}: ligand') for c, (o, r) in enumerate(zip(lig_res_offsets, lr))]
        rro = [_residue_table(o, len(r), f'complex {c}: receptor') for c, (o, r) in enumerate(zip(rec_res_offsets, rr))]
        lca = [_ca_rows(None if lig_names is None else lig_names[c], o, len(r), f'complex {c}: ligand')
               for c, (o, r) in enumerate(zip(lro, lr))]
        rca = [_ca_rows(None if rec_names is None else rec_names[c], o, len(r), f'complex {c}: receptor')
               for c, (o, r) in enumerate(zip(rro, rr))]
        self.n, self.dev, self.n_points = n, torch.device(dev), int(n_points)
        _require_device(torch.empty(0, device=self.dev), 'depth inputs')
        sphere = sphere_points(self.n_points)
        self.lig_atom_off, self.rec_atom_off = _offsets([len(r) for r in lr]), _offsets([len(r) for r in rr])
        self.lig_res_off, self.rec_res_off = _offsets([len(o) - 1 for o in lro]), _offsets([len(o) - 1 for o in rro])
        self._off = tuple(a.ctypes.data_as(C.c_void_p) for a in (self.lig_atom_off, self.rec_atom_off, self.lig_res_off,
                                                                  self.rec_res_off))
        Al, Ar, Rl, Rr = (int(a[-1]) for a in (self.lig_atom_off, self.rec_atom_off, self.lig_res_off, self.rec_res_off))
        self.sizes = (Al, Ar, Rl, Rr)
        # one staging buffer, one upload: fp64 sphere table | int32 first rows of the ligand, of the receptor residues, CA
        # rows of the ligand, of the receptor residues | fp32 radii of the ligand, of the receptor atoms
        nb_s, nb_f = 24 * self.n_points, 4 * (2 * (Rl + Rr) + 2)
        host = _staging(nb_s + nb_f + 4 * (Al + Ar), torch.uint8, self.dev)
        h = host.numpy()
        h[:nb_s].view(np.float64)[:] = sphere.reshape(-1)
        ints = h[nb_s:nb_s + nb_f].view(np.int32)
        ints[:Rl + 1] = np.concatenate([o[:-1] + int(a) for o, a in zip(lro, self.lig_atom_off)] + [[Al]])
        ints[Rl + 1:Rl + Rr + 2] = np.concatenate([o[:-1] + int(a) for o, a in zip(rro, self.rec_atom_off)] + [[Ar]])
        ints[Rl + Rr + 2:2 * Rl + Rr + 2] = np.concatenate([np.where(k >= 0, k + int(a), -1) for k, a in zip(lca, self.lig_atom_off)])
        ints[2 * Rl + Rr + 2:] = np.concatenate([np.where(k >= 0, k + int(a), -1) for k, a in zip(rca, self.rec_atom_off)])
        h[nb_s + nb_f:].view(np.float32)[:] = np.concatenate(lr + rr)
        self.tables = host.to(self.dev, non_blocking=True)
        self.sphere = self.tables[:nb_s].view(torch.float64).view(self.n_points, 3)
        ints = self.tables[nb_s:nb_s + nb_f].view(torch.int32)
        self.lig_first, self.rec_first = ints[:Rl + 1], ints[Rl + 1:Rl + Rr + 2]
        self.lig_ca, self.rec_ca = ints[Rl + Rr + 2:2 * Rl + Rr + 2], ints[2 * Rl + Rr + 2:]
        rad = self.tables[nb_s + nb_f:].view(torch.float32)
        self.lig_radii, self.rec_radii = rad[:Al], rad[Al:]
        self.wsb = lib.eqd_dock_depth_workspace_bytes(n, *self._off, self.n_points)
        if self.wsb == 0:
            check(2)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=self.dev)
        with _lib.device_guard(self.dev):
            check(lib.eqd_dock_depth_init(n, *self._off, self.n_points, _lib.ptr(self.ws), C.c_size_t(self.wsb),
                                          _stream(self.dev)))

    def outputs(self):
        """Freshly allocated output buffers of one eval: (atom depths [A_l + A_r][4] fp64: s_alone, s_complex, depth_alone,
        depth_complex; residue depths [R_l + R_r][4] fp64: mean alone, mean in complex, CA alone, CA in complex; rows
        [C][16] fp64); the ligand's rows come first in the first two."""
        Al, Ar, Rl, Rr = self.sizes
        return (torch.empty(Al + Ar, 4, dtype=torch.float64, device=self.dev),
                torch.empty(Rl + Rr, 4, dtype=torch.float64, device=self.dev),
                torch.empty(self.n, DEPTH_COLS, dtype=torch.float64, device=self.dev))

    def eval(self, lig, rec, depth, res_depth, rows, probe=1.4, prune=None):
        """Enqueue the depth pass on the current stream: lig [A_l][3], rec [A_r][3] fp32 contiguous, the buffers of
        `outputs()`.  No synchronisation, no allocation, no copy."""
        Al, Ar, Rl, Rr = self.sizes
        prune = depth_pruning_enabled() if prune is None else bool(prune)
        with _lib.device_guard(self.dev):
            check(_dock.eqd_dock_depth_eval(self.n, *self._off, _lib.ptr(lig), _lib.ptr(rec), _lib.ptr(self.lig_radii),
                                            _lib.ptr(self.rec_radii), _lib.ptr(self.lig_first), _lib.ptr(self.rec_first),
                                            _lib.ptr(self.lig_ca), _lib.ptr(self.rec_ca), _lib.ptr(self.sphere),
                                            self.n_points, C.c_double(float(probe)), int(prune), _lib.ptr(depth[:Al]),
                                            _lib.ptr(depth[Al:]), _lib.ptr(res_depth[:Rl]), _lib.ptr(res_depth[Rl:]),
                                            _lib.ptr(rows), _lib.ptr(self.ws), C.c_size_t(self.wsb), _stream(self.dev)))
        return rows


def residue_depth_batch(lig_list, rec_list, lig_radii=None, rec_radii=None, lig_res_offsets=None, rec_res_offsets=None,
                        lig_names=None, rec_names=None, probe=1.4, n_points=96, plan=None):
    """Depth of every heavy atom and residue of C complexes below its protein's surface, alone and in complex, in one
    device pass (eqd_dock_depth_*; the definitions are in include/equidock_dock.h): the distance to the nearest surface
    vertex, a vertex being the van-der-Waals contact point of a Shrake-Rupley sphere point (`n_points` per atom, probe of
    `probe` Angstrom) that stays exposed.  This is the contact patch of the solvent-excluded surface, not MSMS's surface:
    re-entrant patches are not modelled.  It needs no native structure.  The lists hold device tensors [n_c, 3] of heavy
    atoms; per complex (host arrays, as `atom_radii` / `atom_table` return them) the radii [n_c] (finite, > 0), the residue
    offsets [n_res + 1] into its own rows of each side and optionally the atom names [n_c] (for the CA depth; without them
    it is NaN) - or a `plan` (DepthPlan) that already holds them.  fp64 on the device from the fp32 rows; a complex's
    results are bit-identical alone, in any batch and from run to run.

    Returns a dict of device tensors: DEPTH_KEYS (float64 [C]: depth_ligand / depth_receptor - mean atom depth alone -,
    depth_complex, max_depth_ligand / _receptor / _complex, depth_gain_ligand / _receptor - mean of depth in complex minus
    depth alone -, deepened_atoms_ligand / _receptor, deepened_residues_ligand / _receptor, vertices_alone,
    vertices_complex, skipped_groups, flags), `rows`, the raw [C][16] buffer, `lig_depth` / `rec_depth` (float64 [A][4]:
    s_alone, s_complex, depth_alone, depth_complex), `lig_res_depth` / `rec_res_depth` (float64 [R][4]: mean alone, mean in
    complex, CA alone, CA in complex) and `plan`.  One upload of the small tables (when no plan is given), one launch
    sequence; apart from the tile-table copy of the workspace's init the call does not synchronise and downloads nothing."""
    ligs, recs = list(lig_list), list(rec_list)
    n = len(ligs)
    if n != len(recs):
        raise ValueError(f"{n} ligands for {len(recs)} receptors")
    if n == 0:
        raise ValueError("residue_depth_batch: no complexes")
    ligs, recs = _meter_rows(ligs, 'ligand'), _meter_rows(recs, 'receptor')
    dev = ligs[0].device
    if plan is None:
        if lig_radii is None or rec_radii is None or lig_res_offsets is None or rec_res_offsets is None:
            raise ValueError("residue_depth_batch: radii and residue offsets of both sides (or a plan) are needed")
        plan = DepthPlan(list(lig_res_offsets), list(rec_res_offsets), list(lig_radii), list(rec_radii), dev,
                         n_points=n_points, lig_names=None if lig_names is None else list(lig_names),
                         rec_names=None if rec_names is None else list(rec_names))
    if plan.n != n:
        raise ValueError(f"the plan holds {plan.n} complexes, the lists {n}")
    for c in range(n):
        nl, nr = int(plan.lig_atom_off[c + 1] - plan.lig_atom_off[c]), int(plan.rec_atom_off[c + 1] - plan.rec_atom_off[c])
        if ligs[c].shape[0] != nl or recs[c].shape[0] != nr:
            raise ValueError(f"complex {c}: {ligs[c].shape[0]} ligand and {recs[c].shape[0]} receptor rows for tables of "
                             f"{nl} and {nr} atoms")
    depth, res_depth, rows = plan.outputs()
    plan.eval(torch.cat(ligs, 0), torch.cat(recs, 0), depth, res_depth, rows, probe=probe)
    Al, Rl = plan.sizes[0], plan.sizes[2]
    res = {k: rows[:, i] for i, k in enumerate(DEPTH_KEYS)}
    res.update(rows=rows, lig_depth=depth[:Al], rec_depth=depth[Al:], lig_res_depth=res_depth[:Rl],
               rec_res_depth=res_depth[Rl:], plan=plan)
    return res


def _average_ranks(v):
    order = np.argsort(v, kind='stable')
    s = v[order]
    start = np.concatenate(([True], s[1:] != s[:-1]))
    first = np.nonzero(start)[0]
    last = np.concatenate((first[1:], [len(v)])) - 1
    mean = 0.5 * (first + last) + 1.0                           # a run of ties takes the mean of its 1-based positions
    ranks = np.empty(len(v), dtype=np.float64)
    ranks[order] = mean[np.cumsum(start) - 1]
    return ranks


def spearman(a, b):
    """Spearman's rank correlation of two equally long vectors (the statistic of scipy.stats.spearmanr): float64 on the
    host, average ranks for ties, then Pearson's correlation of the ranks; NaN for fewer than two values or when one input
    is constant."""
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64).reshape(-1)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64).reshape(-1)
    if len(a) != len(b):
        raise ValueError(f"spearman: {len(a)} values for {len(b)}")
    if len(a) < 2:
        return float('nan')
    ra, rb = _average_ranks(a), _average_ranks(b)
    da, db = ra - ra.mean(), rb - rb.mean()
    den = np.sqrt((da * da).sum() * (db * db).sum())
    if not den > 0.0:
        return float('nan')
    return float((da * db).sum() / den)


# ---- batched graph construction -------------------------------------------------------------------------------------
GRAPH_KEYS =('x', 'res_feat', 'mu_r_norm', 'src', 'dst', 'he')
last_graph_stats = {}      # of the latest protein_graphs_batch call: proteins, residues, edges, pairs, pruned_pairs, pruning


def graph_pruning_enabled():
    """EQD_DOCK_GRAPH_PRUNE=0 turns the centroid-distance pruning of the distance phase off (same results either way)."""
    return os.environ.get('EQD_DOCK_GRAPH_PRUNE', '1') != '0'


def _int32_offsets(sizes, what):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    if off[-1] > np.iinfo(np.int32).max:
        raise _lib.EquidockHipError(f"{int(off[-1])} {what} do not fit int32 offsets: split the batch")
    return np.ascontiguousarray(off.astype(np.int32))


def _staging(n, dtype, dev):
    """Host buffer of one upload or download: pinned when the device is a GPU (torch caches pinned blocks)."""
    return torch.empty(n, dtype=dtype, pin_memory=dev.type == 'cuda')


def protein_graphs_batch(proteins, cutoff, max_neighbor, device, residue_loc_is_alphaC=True):
    """featurize.protein_graph for a list of (residues, bound_ca) proteins in one device pass (eqd_dock_graph_*): host
    preparation per protein as there (local frames, alignment onto the bound C-alpha array, ragged atoms, residue ids),
    then one upload per dtype, one launch per phase for ALL proteins, one read of the counts and one download per dtype.
    Returns one dict per protein with the keys and dtypes of protein_graph (device tensors, bit-identical to it) plus
    'host': the same six arrays as numpy views of the downloaded buffers, which graph.batch_pairs takes as they are.
    A residue without a neighbour under the cutoff raises ValueError naming the protein's index in the batch."""
    global last_graph_stats
    lib = load_dock_library()
    proteins = list(proteins)
    K = int(max_neighbor)
    if K < 1 or K > 64:
        raise ValueError("max_neighbor must be in 1..64")
    if not proteins:
        return []
    dev = torch.device(device)
    _require_device(torch.empty(0, device=dev), 'protein graph inputs')
    P = len(proteins)
    prep = []
    for residues, bound_ca in proteins:
        loc, n_i, u_i, v_i = FZ.local_frames(residues, residue_loc_is_alphaC)
        R, t = FZ.rigid_transform_kabsch_3d(loc.T, np.asarray(bound_ca).T)
        x = ((R @ loc.T) + t).T                     # float64 from here on, as in the reference
        n_i, u_i, v_i = (R @ n_i.T).T, (R @ u_i.T).T, (R @ v_i.T).T
        atoms, off = FZ.atoms_ragged(residues)
        res = np.asarray([FZ.residue_type_id(r.resname) for r in residues], dtype=np.float32)
        prep.append((atoms, off, x, n_i, u_i, v_i, res))
    res_off = _int32_offsets([len(q[6]) for q in prep], 'residues')
    patom_off = _int32_offsets([q[0].shape[0] for q in prep], 'atoms')
    if 3 * int(patom_off[-1]) > np.iinfo(np.int32).max:
        raise _lib.EquidockHipError(f"{int(patom_off[-1])} atoms do not fit int32 offsets: split the batch")
    Rn, A = int(res_off[-1]), int(patom_off[-1])
    ro, po = res_off.ctypes.data_as(C.c_void_p), patom_off.ctypes.data_as(C.c_void_p)
    wsb = lib.eqd_dock_graph_workspace_bytes(P, ro, po, K)
    if wsb == 0:
        check(2)
    # one staging buffer and one upload per dtype: fp32 = atoms | x | residue ids, fp64 = x | n | u | v, int32 = atom offsets
    h32, h64, hi = _staging(3 * A + 4 * Rn, torch.float32, dev), _staging(12 * Rn, torch.float64, dev), _staging(Rn + 1, torch.int32, dev)
    a32, a64, ai = h32.numpy(), h64.numpy().reshape(4, Rn, 3), hi.numpy()
    ai[0] = 0
    for p, (atoms, off, x, n_i, u_i, v_i, res) in enumerate(prep):
        r0, r1, a0, a1 = int(res_off[p]), int(res_off[p + 1]), int(patom_off[p]), int(patom_off[p + 1])
        a32[3 * a0:3 * a1] = atoms.reshape(-1)
        a32[3 * A + 3 * r0:3 * A + 3 * r1] = x.astype(np.float32).reshape(-1)
        a32[3 * A + 3 * Rn + r0:3 * A + 3 * Rn + r1] = res
        for q, v in enumerate((x, n_i, u_i, v_i)):
            a64[q, r0:r1] = v
        ai[r0 + 1:r1 + 1] = off[1:] + a0
    d32, d64, di = (h.to(dev, non_blocking=True) for h in (h32, h64, hi))
    xs = d64.view(4, Rn, 3)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    deg = torch.empty(Rn, dtype=torch.int32, device=dev)
    mu = torch.empty(Rn, 5, dtype=torch.float32, device=dev)
    counts = torch.empty(2 * P + 2, dtype=torch.int32, device=dev)      # pruned pairs | edge offsets [P + 1] | no-neighbour [P]
    prune = graph_pruning_enabled()
    st = _stream(dev)
    with _lib.device_guard(dev):
        check(lib.eqd_dock_graph_init(P, ro, po, K, _lib.ptr(ws), C.c_size_t(wsb), st))
        check(lib.eqd_dock_graph_select(P, ro, po, _lib.ptr(d32), _lib.ptr(di), _lib.ptr(xs[0]), C.c_double(float(cutoff)), K,
                                        int(prune), _lib.ptr(deg), _lib.ptr(counts[1:]), _lib.ptr(mu), _lib.ptr(counts[P + 2:]),
                                        _lib.ptr(counts), _lib.ptr(ws), C.c_size_t(wsb), st))
    cnt = counts.cpu().numpy()                                          # device-to-host synchronisation 1 of 2
    eoff, lonely = cnt[1:P + 2], cnt[P + 2:]
    if (lonely >= 0).any():
        # the reference asserts here (protein_utils.py:354, `assert len(valid_src) > 0`), and mu_r_norm would be 0 / 0
        p = int(np.nonzero(lonely >= 0)[0][0])
        raise ValueError(f"protein {p} of the batch: residue {int(lonely[p])} has no neighbour closer than cutoff={cutoff}: "
                         "the reference asserts on such graphs (src/utils/protein_utils.py:354)")
    E = int(eoff[P])
    sd = torch.empty(2, E, dtype=torch.int32, device=dev)
    he = torch.empty(E, 27, dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        check(lib.eqd_dock_graph_edges(P, ro, po, K, _lib.ptr(xs[0]), _lib.ptr(xs[1]), _lib.ptr(xs[2]), _lib.ptr(xs[3]),
                                       _lib.ptr(sd[0]), _lib.ptr(sd[1]), _lib.ptr(he), _lib.ptr(ws), C.c_size_t(wsb), st))
    if dev.type == 'cuda':
        of, oi = _staging(27 * E + 5 * Rn, torch.float32, dev), _staging(2 * E, torch.int32, dev)
        of[:27 * E].copy_(he.view(-1), non_blocking=True)
        of[27 * E:].copy_(mu.view(-1), non_blocking=True)
        oi.copy_(sd.view(-1), non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()                    # device-to-host synchronisation 2 of 2
        he_h, mu_h, sd_h = of[:27 * E].numpy().reshape(E, 27), of[27 * E:].numpy().reshape(Rn, 5), oi.numpy().reshape(2, E)
    else:
        he_h, mu_h, sd_h = he.numpy(), mu.numpy(), sd.numpy()
    x_d, res_d = d32[3 * A:3 * A + 3 * Rn].view(Rn, 3), d32[3 * A + 3 * Rn:].view(Rn, 1)
    x_h, res_h = a32[3 * A:3 * A + 3 * Rn].reshape(Rn, 3), a32[3 * A + 3 * Rn:].reshape(Rn, 1)
    out = []
    for p in range(P):
        r0, r1, e0, e1 = int(res_off[p]), int(res_off[p + 1]), int(eoff[p]), int(eoff[p + 1])
        out.append({'x': x_d[r0:r1], 'res_feat': res_d[r0:r1], 'mu_r_norm': mu[r0:r1], 'src': sd[0, e0:e1],
                    'dst': sd[1, e0:e1], 'he': he[e0:e1],
                    'host': {'x': x_h[r0:r1], 'res_feat': res_h[r0:r1], 'mu_r_norm': mu_h[r0:r1], 'src': sd_h[0, e0:e1],
                             'dst': sd_h[1, e0:e1], 'he': he_h[e0:e1]}})
    n = np.diff(res_off).astype(np.int64)
    last_graph_stats = {'proteins': P, 'residues': Rn, 'edges': E, 'pairs': int((n * (n - 1) // 2).sum()),
                        'pruned_pairs': int(cnt[0]), 'pruning': prune}
    return out


# ---- model + files ------------------------------------------------------------------------------------------------
def load_checkpoint(path, device):
    """Rigid_Body_Docking_Net from a reference checkpoint {'args', 'state_dict'} (src/inference_rigid.py:97-112): the
    `args` keys the drop-in reads are taken from the checkpoint, the rest from config.published_args().  The whole
    checkpoint `args` stays available as `net.checkpoint_args` (graph_cutoff, graph_max_neighbor)."""
    from .model import Rigid_Body_Docking_Net
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    if not isinstance(ckpt, dict) or 'args' not in ckpt or 'state_dict' not in ckpt:
        raise ValueError(f"{path}: expected a dict with 'args' and 'state_dict'")
    device = torch.device(device)
    base = config.published_args()
    args = {k: ckpt['args'].get(k, v) for k, v in base.items()}
    args.update(debug=False, device=device)
    net = Rigid_Body_Docking_Net(args)
    net.load_state_dict(ckpt['state_dict'])
    net = net.to(device).eval()
    net.checkpoint_args = dict(ckpt['args'])
    return net


def _side(x):
    """(residues, all ATOM coordinates in file order) of a PDB path or a residue list."""
    if isinstance(x, (str, os.PathLike)):
        return FZ.read_pdb_residues(x), INF.read_pdb_atoms(x)
    return list(x), FZ.atoms_ragged(list(x))[0]


def _ca_index(x):
    """Rows of the C-alpha atoms among the all-atom rows of `_side(x)`, by the rule of inference.read_pdb_atoms(ca_only=True)
    (ATOM records whose name field reads CA, in file order)."""
    if isinstance(x, (str, os.PathLike)):
        with open(x) as f:
            names = [line[12:16].strip() for line in f if line.startswith('ATOM')]
    else:
        names = [a.strip() for r in x for a in r.atom_names]
    return np.nonzero(np.asarray(names) == 'CA')[0].astype(np.int64)


def _ca_coords(x):
    """C-alpha coordinates [n, 3] float32 of a PDB path or a residue list (same rule)."""
    if isinstance(x, (str, os.PathLike)):
        return INF.read_pdb_atoms(x, ca_only=True)
    x = list(x)
    return np.ascontiguousarray(FZ.atoms_ragged(x)[0][_ca_index(x)], dtype=np.float32).reshape(-1, 3)


def _chunk_metrics(chunk, truths, first, final_lig, rec_atoms, cutoff, dev):
    """The metrics stage of dock_complexes for one chunk: C-alpha rows of the final ligands and of the receptors taken on
    the device by an index built on the host, one rmsd_metrics_batch, ONE download of the [C][8] rows."""
    li, ri, gts = [], [], []
    for k, ((lig_in, rec_in), gt) in enumerate(zip(chunk, truths)):
        li.append(_ca_index(lig_in))
        ri.append(_ca_index(rec_in))
        gts.append(_ca_coords(gt))
        if len(li[-1]) != len(gts[-1]) or len(li[-1]) == 0:
            raise ValueError(f"complex {first + k}: the ligand has {len(li[-1])} C-alpha atoms, its ground truth {len(gts[-1])}")
        if len(ri[-1]) == 0:
            raise ValueError(f"complex {first + k}: the receptor has no C-alpha atom")
    n_idx, n_gt = sum(len(a) for a in li + ri), sum(len(a) for a in gts)
    hidx, hgt = _staging(n_idx, torch.int64, dev), _staging(3 * n_gt, torch.float32, dev)
    hidx.numpy()[:] = np.concatenate(li + ri)
    hgt.numpy()[:] = np.concatenate(gts, 0).reshape(-1)
    didx, dgt = hidx.to(dev, non_blocking=True), hgt.to(dev, non_blocking=True).view(-1, 3)
    ioff = np.concatenate([[0], np.cumsum([len(a) for a in li + ri])])
    goff = np.concatenate([[0], np.cumsum([len(a) for a in gts])])
    n = len(chunk)
    lig_pred = [final_lig[k].index_select(0, didx[ioff[k]:ioff[k + 1]]) for k in range(n)]
    rec_true = [rec_atoms[k].index_select(0, didx[ioff[n + k]:ioff[n + k + 1]]) for k in range(n)]
    lig_true = [dgt[goff[k]:goff[k + 1]] for k in range(n)]
    return rmsd_metrics_batch(lig_pred, lig_true, rec_true, cutoff=cutoff, interface=True)['metrics'].cpu().numpy()


def _chunk_heavy_rows(chunk, truths, first, final_lig, rec_atoms, dev):
    """The heavy-atom rows of a chunk's final ligands and receptors, taken on the device by an index built on the host, and
    the heavy atoms of the ground-truth ligands in one upload: (ligand tables, receptor tables - as atom_table returns them
    -, model ligands, native ligands, receptors).  A ligand whose heavy-atom names differ from its ground truth's raises
    ValueError naming the complex."""
    lig_t, rec_t, gts = [], [], []
    for k, ((lig_in, rec_in), gt) in enumerate(zip(chunk, truths)):
        lig_t.append(atom_table(lig_in))
        rec_t.append(atom_table(rec_in))
        gts.append(atom_table(gt))
        if len(lig_t[-1][4]) == 0 or len(rec_t[-1][4]) == 0:
            raise ValueError(f"complex {first + k}: a side without a heavy atom")
        if len(lig_t[-1][4]) != len(gts[-1][4]) or (lig_t[-1][4] != gts[-1][4]).any():
            raise ValueError(f"complex {first + k}: the ligand's heavy-atom names differ from its ground truth's "
                             f"({len(lig_t[-1][4])} and {len(gts[-1][4])} heavy atoms)")
    n = len(chunk)
    idx = [t[1] for t in lig_t + rec_t]
    n_idx, n_gt = sum(len(a) for a in idx), sum(len(t[0]) for t in gts)
    hidx, hgt = _staging(n_idx, torch.int64, dev), _staging(3 * n_gt, torch.float32, dev)
    hidx.numpy()[:] = np.concatenate(idx)
    hgt.numpy()[:] = np.concatenate([t[0] for t in gts], 0).reshape(-1)
    didx, dgt = hidx.to(dev, non_blocking=True), hgt.to(dev, non_blocking=True).view(-1, 3)
    ioff = np.concatenate([[0], np.cumsum([len(a) for a in idx])])
    goff = np.concatenate([[0], np.cumsum([len(t[0]) for t in gts])])
    lig_pred = [final_lig[k].index_select(0, didx[ioff[k]:ioff[k + 1]]) for k in range(n)]
    rec_true = [rec_atoms[k].index_select(0, didx[ioff[n + k]:ioff[n + k + 1]]) for k in range(n)]
    lig_true = [dgt[goff[k]:goff[k + 1]] for k in range(n)]
    return lig_t, rec_t, lig_pred, lig_true, rec_true


def _chunk_quality(chunk, truths, first, final_lig, rec_atoms, cuts, dev):
    """The quality stage of dock_complexes for one chunk: the heavy-atom rows of the final ligands and of the receptors
    taken on the device by an index built on the host, one pose_quality_batch (the model's receptor is the receptor given),
    ONE download of the [C][16] rows - a download of its own, after the meter's."""
    lig_t, rec_t, lig_pred, lig_true, rec_true = _chunk_heavy_rows(chunk, truths, first, final_lig, rec_atoms, dev)
    q = pose_quality_batch(lig_pred, lig_true, rec_true, [t[2] for t in lig_t], [t[2] for t in rec_t], [t[3] for t in lig_t],
                           [t[3] for t in rec_t], contact_cutoff=cuts[0], interface_cutoff=cuts[1], clash_cutoff=cuts[2])
    return q['quality'].cpu().numpy()


def _chunk_lddt(chunk, truths, first, final_lig, rec_atoms, radius, dev):
    """The lDDT stage of dock_complexes for one chunk: the rows of `_chunk_heavy_rows`, one lddt_batch (the model's receptor
    is the receptor given), ONE download of the [C][16] rows."""
    lig_t, rec_t, lig_pred, lig_true, rec_true = _chunk_heavy_rows(chunk, truths, first, final_lig, rec_atoms, dev)
    return lddt_batch(lig_pred, lig_true, rec_true, [t[2] for t in lig_t], [t[2] for t in rec_t],
                      inclusion_radius=radius)['rows'].cpu().numpy()


def _chunk_surface(chunk, truths, first, final_lig, rec_atoms, probe, n_points, dev):
    """The surface stage of dock_complexes for one chunk: the heavy-atom rows of the final ligands and of the receptors
    taken on the device by an index built on the host, one surface_area_batch - with `truths` the native ligands ride in
    the SAME batch as C more complexes against the same receptors -, ONE download of the [C or 2 C][12] rows."""
    lig_t, rec_t = [], []
    for k, (lig_in, rec_in) in enumerate(chunk):
        lig_t.append(atom_table(lig_in) + (atom_radii(lig_in),))
        rec_t.append(atom_table(rec_in) + (atom_radii(rec_in),))
        if len(lig_t[-1][4]) == 0 or len(rec_t[-1][4]) == 0:
            raise ValueError(f"complex {first + k}: a side without a heavy atom")
    gts = []
    for k, gt in enumerate(truths or []):
        gts.append(atom_table(gt) + (atom_radii(gt),))
        if len(gts[-1][4]) == 0:
            raise ValueError(f"complex {first + k}: a ground-truth ligand without a heavy atom")
    n = len(chunk)
    idx = [t[1] for t in lig_t + rec_t]
    hidx = _staging(sum(len(a) for a in idx), torch.int64, dev)
    hidx.numpy()[:] = np.concatenate(idx)
    didx = hidx.to(dev, non_blocking=True)
    ioff = np.concatenate([[0], np.cumsum([len(a) for a in idx])])
    ligs = [final_lig[k].index_select(0, didx[ioff[k]:ioff[k + 1]]) for k in range(n)]
    recs = [rec_atoms[k].index_select(0, didx[ioff[n + k]:ioff[n + k + 1]]) for k in range(n)]
    if gts:
        hgt = _staging(3 * sum(len(t[0]) for t in gts), torch.float32, dev)
        hgt.numpy()[:] = np.concatenate([t[0] for t in gts], 0).reshape(-1)
        dgt = hgt.to(dev, non_blocking=True).view(-1, 3)
        goff = np.concatenate([[0], np.cumsum([len(t[0]) for t in gts])])
        ligs += [dgt[goff[k]:goff[k + 1]] for k in range(n)]
        recs += recs
    s = surface_area_batch(ligs, recs, [t[5] for t in lig_t + gts], [t[5] for t in rec_t] * (2 if gts else 1),
                           [t[2] for t in lig_t + gts], [t[2] for t in rec_t] * (2 if gts else 1), probe=probe,
                           n_points=n_points)
    return s['rows'].cpu().numpy()


def _chunk_depth(chunk, first, final_lig, rec_atoms, probe, n_points, dev):
    """The depth stage of dock_complexes for one chunk: the heavy-atom rows of the final ligands and of the receptors (the
    rows `_chunk_surface` takes) taken on the device by an index built on the host, one residue_depth_batch, ONE download
    of the [C][16] rows."""
    lig_t, rec_t = [], []
    for k, (lig_in, rec_in) in enumerate(chunk):
        lig_t.append(atom_table(lig_in) + (atom_radii(lig_in),))
        rec_t.append(atom_table(rec_in) + (atom_radii(rec_in),))
        if len(lig_t[-1][4]) == 0 or len(rec_t[-1][4]) == 0:
            raise ValueError(f"complex {first + k}: a side without a heavy atom")
    n = len(chunk)
    idx = [t[1] for t in lig_t + rec_t]
    hidx = _staging(sum(len(a) for a in idx), torch.int64, dev)
    hidx.numpy()[:] = np.concatenate(idx)
    didx = hidx.to(dev, non_blocking=True)
    ioff = np.concatenate([[0], np.cumsum([len(a) for a in idx])])
    ligs = [final_lig[k].index_select(0, didx[ioff[k]:ioff[k + 1]]) for k in range(n)]
    recs = [rec_atoms[k].index_select(0, didx[ioff[n + k]:ioff[n + k + 1]]) for k in range(n)]
    d = residue_depth_batch(ligs, recs, [t[5] for t in lig_t], [t[5] for t in rec_t], [t[2] for t in lig_t],
                            [t[2] for t in rec_t], lig_names=[t[4] for t in lig_t], rec_names=[t[4] for t in rec_t],
                            probe=probe, n_points=n_points)
    return d['rows'].cpu().numpy()


def _sync(dev):
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)


def _chunk_graphs(chunk, cutoff, max_neighbor, dev):
    """The graphs stage of dock_complexes for one chunk in one device pass: (pairs for graph.batch_pairs - host views, no
    further download -, ligand atoms, receptor atoms); the atoms of all complexes go up in one copy."""
    prots, sides = [], []
    for lig_in, rec_in in chunk:
        lig_res, lig_all = _side(lig_in)
        rec_res, rec_all = _side(rec_in)
        lig, rec, lig_ca, rec_ca = FZ.preprocess_unbound_bound(lig_res, rec_res, inference=True)
        prots += [(lig, lig_ca), (rec, rec_ca)]
        sides += [lig_all, rec_all]
    gs = [g['host'] for g in protein_graphs_batch(prots, cutoff, max_neighbor, dev)]
    pairs = [(dict(gs[2 * i], new_x=gs[2 * i]['x']), gs[2 * i + 1]) for i in range(len(chunk))]
    aoff = _int32_offsets([len(a) for a in sides], 'atoms')
    hall = _staging(3 * int(aoff[-1]), torch.float32, dev)
    for i, a in enumerate(sides):
        hall.numpy()[3 * aoff[i]:3 * aoff[i + 1]] = np.asarray(a, dtype=np.float32).reshape(-1)
    dall = hall.to(dev, non_blocking=True).view(-1, 3)
    return (pairs, [dall[aoff[2 * i]:aoff[2 * i + 1]] for i in range(len(chunk))],
            [dall[aoff[2 * i + 1]:aoff[2 * i + 2]] for i in range(len(chunk))])


def dock_complexes(net, complexes, remove_clashes=True, max_complexes_per_batch=None, device=None, cutoff=30.0,
                   max_neighbor=10, sigma=8.0, surface_ct=8.0, loss_stop=0.5, max_it=2000, check_every=50,
                   batched_graphs=True, ground_truth=None, interface_cutoff=8.0, quality=False,
                   quality_cutoffs=(5.0, 10.0, 3.0), surface=False, surface_probe=1.4, surface_points=96, lddt=False,
                   lddt_radius=15.0, depth=False, depth_probe=1.4, depth_points=96):
    """Dock a list of (ligand, receptor) complexes, each side a PDB path or a list of featurize.Residue (the ligand's
    file / residues in their input pose, the receptor's in the bound pose - the reference's `*_l_b.pdb` and
    `*_r_b_COMPLEX.pdb`).  Per chunk of `max_complexes_per_batch` complexes (all at once by default): graphs on the
    device, one batched eval forward, apply_rigid to every ligand atom, then remove_clashes_batch.  `batched_graphs`: all
    graphs of a chunk from one protein_graphs_batch call (and the chunk's atoms in one upload) instead of a loop over
    the complexes; the results are bit-identical either way.

    Returns one dict per complex: rotation [3, 3], translation [3] (numpy), ligand_atoms_docked (apply_rigid of all ligand
    atoms, before clash removal) and ligand_atoms (after it; the same tensor without clash removal), clash_iterations,
    clash_loss, n_ligand_atoms / n_receptor_atoms, and `batch_seconds`: wall times of the complex's chunk (graphs, model,
    rigid, clashes, total; device-synchronised).

    `ground_truth`: one entry per complex, the ligand in its bound pose (a PDB path or a list of featurize.Residue; the
    receptor's ground truth is the receptor given).  Each chunk then ends with one rmsd_metrics_batch on the C-alpha rows
    of its final ligands (taken on the device) and one download, and the results gain `crmsd`, `irmsd`, `ligand_rmsd`
    (floats; irmsd NaN without a C-alpha pair closer than `interface_cutoff`) and `interface_pairs`; batch_seconds gains
    'metrics'.  A ligand whose C-alpha count differs from its ground truth's raises ValueError.  Without it nothing changes.

    `quality` (needs `ground_truth`): each chunk also ends with one pose_quality_batch over EVERY heavy atom of its final
    ligands (taken on the device; the model's receptor is the receptor given) and one more download, and the results gain
    `dockq`, `fnat`, `fnonnat`, `irmsd_backbone`, `lrmsd` (floats, NaN where undefined), `native_contacts`,
    `model_contacts` and `clashes` (ints); batch_seconds gains 'quality'.  `quality_cutoffs`: contact, interface and clash
    cutoff.  A ligand whose heavy-atom names differ from its ground truth's raises ValueError naming the complex.
    quality=False changes nothing.

    `surface` (needs no ground truth): each chunk ends with one surface_area_batch over EVERY heavy atom of its final
    ligands and receptors (taken on the device; radii by atom_radii, probe `surface_probe`, `surface_points` sphere points)
    and one more download, and the results gain `sasa_ligand`, `sasa_receptor`, `sasa_complex`, `bsa` (floats, square
    Angstrom), `buried_atoms_ligand`, `buried_atoms_receptor`, `buried_residues_ligand` and `buried_residues_receptor`
    (ints); batch_seconds gains 'surface'.  With `ground_truth` the native ligands go into the same batch as C more
    complexes and the results gain `bsa_native`.  surface=False changes nothing.

    `lddt` (needs `ground_truth`): each chunk also ends with one lddt_batch over EVERY heavy atom of its final ligands
    (the rows and the heavy-atom-name check of `quality`; the model's receptor is the receptor given; inclusion radius
    `lddt_radius`, thresholds 0.5, 1, 2 and 4 Angstrom) and one more download, and the results gain `lddt`, `ilddt`
    (floats; ilddt NaN when no inter-chain atom pair of the native is closer than the radius), `lddt_pairs` and
    `ilddt_pairs` (ints: the included ordered atom pairs); batch_seconds gains 'lddt'.  lddt=False changes nothing.

    `depth` (needs no ground truth): each chunk ends with one residue_depth_batch over EVERY heavy atom of its final
    ligands and receptors (the rows of `surface`; radii by atom_radii, probe `depth_probe`, `depth_points` sphere points)
    and one more download, and the results gain `depth_gain_ligand`, `depth_gain_receptor` (floats, Angstrom: the mean
    over the side's atoms of the depth in complex minus the depth alone), `deepened_atoms_ligand` / `_receptor` and
    `deepened_residues_ligand` / `_receptor` (ints); batch_seconds gains 'depth'.  depth=False changes nothing."""
    complexes = list(complexes)
    if quality and ground_truth is None:
        raise ValueError("quality=True needs ground_truth")
    if lddt and ground_truth is None:
        raise ValueError("lddt=True needs ground_truth")
    if ground_truth is not None:
        ground_truth = list(ground_truth)
        if len(ground_truth) != len(complexes):
            raise ValueError(f"{len(ground_truth)} ground-truth ligands for {len(complexes)} complexes")
    dev = torch.device(device) if device is not None else next(net.parameters()).device
    step = len(complexes) if not max_complexes_per_batch else int(max_complexes_per_batch)
    results = []
    was_training = net.training
    net.eval()
    try:
        for b0 in range(0, len(complexes), max(step, 1)):
            chunk = complexes[b0:b0 + step]
            _sync(dev)
            t0 = time.perf_counter()
            if batched_graphs:
                pairs, lig_atoms, rec_atoms = _chunk_graphs(chunk, cutoff, max_neighbor, dev)
            else:
                pairs, lig_atoms, rec_atoms = [], [], []
                for lig_in, rec_in in chunk:
                    lig_res, lig_all = _side(lig_in)
                    rec_res, rec_all = _side(rec_in)
                    lig, rec, lig_ca, rec_ca = FZ.preprocess_unbound_bound(lig_res, rec_res, inference=True)
                    gl, gr = FZ.protein_to_graph_unbound_bound(lig, rec, lig_ca, rec_ca, cutoff=cutoff,
                                                               max_neighbor=max_neighbor, device=dev)
                    pairs.append((dict(gl, new_x=gl['x']), gr))
                    lig_atoms.append(torch.from_numpy(np.ascontiguousarray(lig_all, dtype=np.float32)).to(dev))
                    rec_atoms.append(torch.from_numpy(np.ascontiguousarray(rec_all, dtype=np.float32)).to(dev))
            batch = G.batch_pairs(pairs).to(dev)
            _sync(dev)
            t1 = time.perf_counter()
            with torch.no_grad():
                _, _, _, rots, trs = net(batch, epoch=0)
            _sync(dev)
            t2 = time.perf_counter()
            docked = [INF.apply_rigid(rots[i], trs[i], lig_atoms[i]) for i in range(len(chunk))]
            _sync(dev)
            t3 = time.perf_counter()
            if remove_clashes:
                caps = max_it if np.ndim(max_it) == 0 else list(max_it)[b0:b0 + len(chunk)]
                cl = remove_clashes_batch(docked, rec_atoms, sigma=sigma, surface_ct=surface_ct, loss_stop=loss_stop,
                                          max_it=caps, check_every=check_every)
            else:
                cl = [None] * len(chunk)
            _sync(dev)
            t4 = time.perf_counter()
            times = {'graphs': t1 - t0, 'model': t2 - t1, 'rigid': t3 - t2, 'clashes': t4 - t3, 'total': t4 - t0,
                     'n_complexes': len(chunk)}
            rows = qrows = srows = lrows = drows = None
            if ground_truth is not None:
                final = [cl[i]['positions'] if cl[i] is not None else docked[i] for i in range(len(chunk))]
                rows = _chunk_metrics(chunk, ground_truth[b0:b0 + len(chunk)], b0, final, rec_atoms, interface_cutoff, dev)
                t5 = time.perf_counter()           # (the download has synchronised)
                times.update(metrics=t5 - t4, total=t5 - t0)
                if quality:
                    qrows = _chunk_quality(chunk, ground_truth[b0:b0 + len(chunk)], b0, final, rec_atoms, quality_cutoffs, dev)
                    t6 = time.perf_counter()       # (the download has synchronised)
                    times.update(quality=t6 - t5, total=t6 - t0)
                if lddt:
                    tl = time.perf_counter()       # (every earlier stage has synchronised)
                    lrows = _chunk_lddt(chunk, ground_truth[b0:b0 + len(chunk)], b0, final, rec_atoms, lddt_radius, dev)
                    tm = time.perf_counter()       # (the download has synchronised)
                    times.update(lddt=tm - tl, total=tm - t0)
            if surface:
                final = [cl[i]['positions'] if cl[i] is not None else docked[i] for i in range(len(chunk))]
                ts = time.perf_counter()           # (every earlier stage has synchronised)
                srows = _chunk_surface(chunk, None if ground_truth is None else ground_truth[b0:b0 + len(chunk)], b0, final,
                                       rec_atoms, surface_probe, surface_points, dev)
                te = time.perf_counter()           # (the download has synchronised)
                times.update(surface=te - ts, total=te - t0)
            if depth:
                final = [cl[i]['positions'] if cl[i] is not None else docked[i] for i in range(len(chunk))]
                td = time.perf_counter()           # (every earlier stage has synchronised)
                drows = _chunk_depth(chunk, b0, final, rec_atoms, depth_probe, depth_points, dev)
                tf = time.perf_counter()           # (the download has synchronised)
                times.update(depth=tf - td, total=tf - t0)
            for i in range(len(chunk)):
                results.append({'rotation': rots[i].detach().cpu().numpy(), 'translation': trs[i].detach().cpu().numpy().reshape(3),
                                'ligand_atoms_docked': docked[i],
                                'ligand_atoms': cl[i]['positions'] if cl[i] is not None else docked[i],
                                'clash_iterations': cl[i]['iterations'] if cl[i] is not None else 0,
                                'clash_loss': cl[i]['loss'] if cl[i] is not None else None,
                                'n_ligand_atoms': int(lig_atoms[i].shape[0]), 'n_receptor_atoms': int(rec_atoms[i].shape[0]),
                                'batch_seconds': times})
                if rows is not None:
                    results[-1].update(crmsd=float(rows[i, 2]), irmsd=float(rows[i, 3]), ligand_rmsd=float(rows[i, 0]),
                                       interface_pairs=int(rows[i, 4]))
                if qrows is not None:
                    q = qrows[i]
                    results[-1].update(dockq=float(q[0]), fnat=float(q[1]), fnonnat=float(q[2]), irmsd_backbone=float(q[3]),
                                       lrmsd=float(q[4]), native_contacts=int(q[5]), model_contacts=int(q[6]),
                                       clashes=int(q[11]))
                if srows is not None:
                    s = srows[i]
                    results[-1].update(sasa_ligand=float(s[0]), sasa_receptor=float(s[1]), sasa_complex=float(s[2]),
                                       bsa=float(s[3]), buried_atoms_ligand=int(s[6]), buried_atoms_receptor=int(s[7]),
                                       buried_residues_ligand=int(s[8]), buried_residues_receptor=int(s[9]))
                    if ground_truth is not None:
                        results[-1].update(bsa_native=float(srows[len(chunk) + i, 3]))
                if lrows is not None:
                    results[-1].update(lddt=float(lrows[i, 0]), ilddt=float(lrows[i, 1]), lddt_pairs=int(lrows[i, 4]),
                                       ilddt_pairs=int(lrows[i, 5]))
                if drows is not None:
                    d = drows[i]
                    results[-1].update(depth_gain_ligand=float(d[6]), depth_gain_receptor=float(d[7]),
                                       deepened_atoms_ligand=int(d[8]), deepened_atoms_receptor=int(d[9]),
                                       deepened_residues_ligand=int(d[10]), deepened_residues_receptor=int(d[11]))
    finally:
        net.train(was_training)
    return results


# ---- the surface-feature analysis (src/surface_analysis.py) -----------------------------------------------------------
def surface_feature_analysis(complexes, device, cutoff=30.0, max_neighbor=10, probe=1.4, n_points=96):
    """The reference's src/surface_analysis.py for a list of (ligand, receptor) complexes, each side a PDB path (read with
    featurize.read_pdb_residues) or a list of featurize.Residue: the Spearman correlation, over the graph nodes of each
    side, between the residue's mean depth below its own protein's surface (alone) and -mu_r_norm[:, 4], the widest-scale
    surface-aware node feature.  The graphs of the filtered residues come from ONE protein_graphs_batch, the depths from
    ONE residue_depth_batch over every heavy atom of the UNFILTERED residue lists (tables by atom_table) - the surface is
    the contact patch under the probe, not MSMS's, so the correlations are not the reference's digit for digit.  A graph
    node is matched to its residue of atom_table by counting the residues of the list that have a heavy atom.

    Returns one dict per complex: `spearman_ligand`, `spearman_receptor` (floats), `n_ligand`, `n_receptor` (graph nodes
    matched), `depth_ligand`, `depth_receptor` and `feature_ligand`, `feature_receptor` (float64 numpy vectors, one entry
    per graph node).  A side that cannot be matched - fewer than two residues pass the N / CA / C filter, a side of its
    complex has no heavy atom, or the graph's node count differs - gives NaN and empty vectors; nothing is raised for
    it (the reference skips such files)."""
    dev = torch.device(device)
    sides = []                                      # per side: (residues, filtered, rows of the filtered ones in atom_table)
    for lig_in, rec_in in complexes:
        for x in (lig_in, rec_in):
            res = FZ.read_pdb_residues(x) if isinstance(x, (str, os.PathLike)) else list(x)
            heavy = np.asarray([any(not _is_hydrogen(nm, el) for nm, el in
                                    zip(r.atom_names, r.elements if len(r.elements) == len(r.atom_names) else [''] * len(r.atom_names)))
                                for r in res], dtype=bool)
            table_row = np.cumsum(heavy) - 1        # the residue's entry in atom_table(res), where it has one
            keep = [i for i, r in enumerate(res) if len(r.atom('N')) == 1 and len(r.atom('CA')) == 1 and len(r.atom('C')) == 1]
            sides.append((res, [res[i] for i in keep], table_row[keep] if keep else np.zeros(0, dtype=np.int64)))
    n = len(sides) // 2
    graphed = [k for k, s in enumerate(sides) if len(s[1]) >= 2]
    graphs = dict(zip(graphed, protein_graphs_batch([(sides[k][1], FZ.alpha_carbon_array(sides[k][1])) for k in graphed], cutoff,
                                                    max_neighbor, dev)))
    tabs = [atom_table(s[0]) + (atom_radii(s[0]),) for s in sides]
    batch = [c for c in range(n) if len(tabs[2 * c][0]) > 0 and len(tabs[2 * c + 1][0]) > 0]
    res_depth = {}
    if batch:
        lt, rt = [tabs[2 * c] for c in batch], [tabs[2 * c + 1] for c in batch]
        coords = np.concatenate([t[0] for t in lt + rt], 0)
        h = _staging(coords.size, torch.float32, dev)
        h.numpy()[:] = coords.reshape(-1)
        d = h.to(dev, non_blocking=True).view(-1, 3)
        off = np.concatenate([[0], np.cumsum([len(t[0]) for t in lt + rt])])
        m = len(batch)
        out = residue_depth_batch([d[off[k]:off[k + 1]] for k in range(m)], [d[off[m + k]:off[m + k + 1]] for k in range(m)],
                                  [t[5] for t in lt], [t[5] for t in rt], [t[2] for t in lt], [t[2] for t in rt],
                                  lig_names=[t[4] for t in lt], rec_names=[t[4] for t in rt], probe=probe, n_points=n_points)
        both = torch.cat((out['lig_res_depth'][:, 0], out['rec_res_depth'][:, 0])).cpu().numpy()     # the one download
        roff = np.concatenate([[0], np.cumsum([len(t[2]) - 1 for t in lt + rt])])
        for k, c in enumerate(batch):
            res_depth[2 * c] = both[roff[k]:roff[k + 1]]
            res_depth[2 * c + 1] = both[roff[m + k]:roff[m + k + 1]]
    results = []
    for c in range(n):
        r = {}
        for k, tag in ((2 * c, 'ligand'), (2 * c + 1, 'receptor')):
            depth, feat = np.zeros(0), np.zeros(0)
            if k in graphs and k in res_depth and graphs[k]['host']['mu_r_norm'].shape[0] == len(sides[k][2]):
                depth = np.ascontiguousarray(res_depth[k][sides[k][2]], dtype=np.float64)
                feat = -np.asarray(graphs[k]['host']['mu_r_norm'][:, 4], dtype=np.float64)
            r.update({f'spearman_{tag}': spearman(depth, feat), f'n_{tag}': len(depth), f'depth_{tag}': depth,
                      f'feature_{tag}': feat})
        results.append(r)
    return results


# ---- command line -------------------------------------------------------------------------------------------------
def _stats(v):
    a = np.asarray(v, dtype=np.float64)
    return float(np.median(a)), float(np.mean(a)), float(np.std(a))


def main(argv=None):
    p = argparse.ArgumentParser(prog='python -m equidock_public_amd.dock',
                                description="EquiDock rigid docking of a directory of complexes (src/inference_rigid.py) "
                                            "with batched graph -> model -> clash removal on the MI355X.")
    p.add_argument('--checkpoint', required=True, help="reference checkpoint {'args', 'state_dict'} (*_model_best.pth)")
    p.add_argument('--input-dir', required=True, help='ligands to dock: <name>_l_b.pdb')
    p.add_argument('--gt-dir', required=True, help='<name>_r_b_COMPLEX.pdb (receptor) and, optionally, '
                                                   '<name>_l_b_COMPLEX.pdb (ground-truth ligand for CRMSD / IRMSD)')
    p.add_argument('--out-dir', required=True)
    p.add_argument('--remove-clashes', action='store_true', help='run the clash-removal loop (src/inference_rigid.py:207-234)')
    p.add_argument('--batch', type=int, default=0, help='complexes per batch (default: all)')
    p.add_argument('--max-it', type=int, default=2000)
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--no-batched-graphs', action='store_true',
                   help='build the graphs in a loop over the complexes instead of one device pass per batch (same results)')
    p.add_argument('--device-metrics', action='store_true',
                   help='CRMSD / IRMSD of every complex from one batched device pass per batch on the docked C-alpha atoms '
                        '(needs every <name>_l_b_COMPLEX.pdb) instead of re-reading the written files on the host')
    p.add_argument('--dockq', action='store_true',
                   help='fnat, LRMSD, backbone iRMSD, DockQ and the clashes of every docked pose from one batched device pass '
                        'per batch over every heavy atom (needs every <name>_l_b_COMPLEX.pdb)')
    p.add_argument('--surface', action='store_true',
                   help='solvent-accessible surface of every docked pose from one batched device pass per batch over every '
                        'heavy atom: buried surface area and buried residues (needs no ground truth; when every '
                        '<name>_l_b_COMPLEX.pdb is present, the native BSA as well)')
    p.add_argument('--lddt', action='store_true',
                   help='lDDT and interface lDDT of every docked pose against its native from one batched device pass per '
                        'batch over every heavy atom (needs every <name>_l_b_COMPLEX.pdb)')
    p.add_argument('--depth', action='store_true',
                   help='residue depth of every docked pose from one batched device pass per batch over every heavy atom: how '
                        'much deeper below the surface binding puts the atoms of each side (needs no ground truth)')
    a = p.parse_args(argv)
    try:
        names = sorted(os.path.basename(f)[:-len('_l_b.pdb')] for f in glob.glob(os.path.join(a.input_dir, '*_l_b.pdb')))
        if not names:
            raise FileNotFoundError(f"no *_l_b.pdb files in {a.input_dir}")
        complexes = []
        for nm in names:
            rec = os.path.join(a.gt_dir, nm + '_r_b_COMPLEX.pdb')
            if not os.path.isfile(rec):
                raise FileNotFoundError(f"{rec} is missing (receptor of {nm})")
            complexes.append((os.path.join(a.input_dir, nm + '_l_b.pdb'), rec))
        truths = None
        if a.device_metrics or a.dockq or a.lddt:
            truths = [os.path.join(a.gt_dir, nm + '_l_b_COMPLEX.pdb') for nm in names]
            for gt in truths:
                if not os.path.isfile(gt):
                    flag = '--device-metrics' if a.device_metrics else '--dockq' if a.dockq else '--lddt'
                    raise FileNotFoundError(f"{gt} is missing ({flag} needs the ground-truth ligand of every complex)")
        if a.surface and truths is None:
            gts = [os.path.join(a.gt_dir, nm + '_l_b_COMPLEX.pdb') for nm in names]
            truths = gts if all(os.path.isfile(g) for g in gts) else None
        os.makedirs(a.out_dir, exist_ok=True)
        dev = torch.device(a.device)
        net = load_checkpoint(a.checkpoint, dev)
        ca = net.checkpoint_args
        t0 = time.perf_counter()
        res = dock_complexes(net, complexes, remove_clashes=a.remove_clashes, max_complexes_per_batch=a.batch or None,
                             device=dev, cutoff=float(ca.get('graph_cutoff', 30.0)),
                             max_neighbor=int(ca.get('graph_max_neighbor', 10)), max_it=a.max_it,
                             batched_graphs=not a.no_batched_graphs, ground_truth=truths, quality=a.dockq, surface=a.surface,
                             lddt=a.lddt, depth=a.depth)
        suffix = '_EQUIDOCK_NO_CLASHES.pdb' if a.remove_clashes else '_EQUIDOCK.pdb'
        crmsd, irmsd, dockq, bsa, bsa_native, ilddt, gain = [], [], [], [], [], [], []
        for nm, (lig_path, rec_path), r in zip(names, complexes, res):
            out = os.path.join(a.out_dir, nm + '_l_b' + suffix)
            INF.write_pdb_coordinates(lig_path, r['ligand_atoms'], out)
            line = (f"{nm}: {r['n_ligand_atoms']} ligand atoms, {r['n_receptor_atoms']} receptor atoms -> {out}")
            if a.remove_clashes:
                line += f"  clash iterations {r['clash_iterations']}, loss {r['clash_loss']:.4f}"
            gt = os.path.join(a.gt_dir, nm + '_l_b_COMPLEX.pdb')
            if a.device_metrics:
                crmsd.append(r['crmsd'])
                irmsd.append(r['irmsd'])
                line += f"  CRMSD {r['crmsd']:.3f}  IRMSD {r['irmsd']:.3f}"
            elif os.path.isfile(gt):
                rec_ca = INF.read_pdb_atoms(rec_path, ca_only=True)
                c, i = INF.complex_and_interface_rmsd(INF.read_pdb_atoms(out, ca_only=True), rec_ca,
                                                      INF.read_pdb_atoms(gt, ca_only=True), rec_ca)
                crmsd.append(c)
                irmsd.append(i)
                line += f"  CRMSD {c:.3f}  IRMSD {i:.3f}"
            if a.dockq:
                dockq.append(r['dockq'])
                line += (f"  DockQ {r['dockq']:.3f}  fnat {r['fnat']:.3f}  LRMSD {r['lrmsd']:.3f}  "
                         f"iRMSD(bb) {r['irmsd_backbone']:.3f}  clashes {r['clashes']}")
            if a.surface:
                bsa.append(r['bsa'])
                line += (f"  BSA {r['bsa']:.1f}  buried residues {r['buried_residues_ligand']} / "
                         f"{r['buried_residues_receptor']}")
                if 'bsa_native' in r:
                    bsa_native.append(r['bsa_native'])
                    line += f"  native BSA {r['bsa_native']:.1f}"
            if a.lddt:
                ilddt.append(r['ilddt'])
                line += f"  lDDT {r['lddt']:.4f}  ilDDT {r['ilddt']:.4f}"
            if a.depth:
                gain.append(r['depth_gain_ligand'])
                line += (f"  depth gain {r['depth_gain_ligand']:.3f} / {r['depth_gain_receptor']:.3f}  deepened residues "
                         f"{r['deepened_residues_ligand']} / {r['deepened_residues_receptor']}")
            print(line, flush=True)
        wall = time.perf_counter() - t0
        print(f"Mean runtime: {wall / len(res):.4f} s per complex ({len(res)} complexes, {wall:.3f} s)")
        if crmsd:
            print("CRMSD median/mean/std: %.3f / %.3f / %.3f" % _stats(crmsd))
            print("IRMSD median/mean/std: %.3f / %.3f / %.3f" % _stats(irmsd))
        if a.dockq:
            dq = np.asarray(dockq, dtype=np.float64)
            ok = dq[~np.isnan(dq)]                  # (DockQ is undefined for a native without a contact)
            print("DockQ median/mean/std: %.3f / %.3f / %.3f" % (_stats(ok) if ok.size else (float('nan'),) * 3))
            print("CAPRI classes (DockQ): incorrect %d  acceptable %d  medium %d  high %d" %
                  (int((ok < 0.23).sum()), int(((ok >= 0.23) & (ok < 0.49)).sum()), int(((ok >= 0.49) & (ok < 0.80)).sum()),
                   int((ok >= 0.80).sum())) + ("  undefined %d" % (dq.size - ok.size) if ok.size < dq.size else ""))
        if bsa:
            print("BSA median/mean/std: %.1f / %.1f / %.1f" % _stats(bsa))
        if bsa_native:
            print("native BSA median/mean/std: %.1f / %.1f / %.1f" % _stats(bsa_native))
        if a.lddt:
            il = np.asarray(ilddt, dtype=np.float64)
            ok = il[~np.isnan(il)]                  # (undefined without an inter-chain atom pair under the radius)
            print("ilDDT median/mean/std: %.4f / %.4f / %.4f" % (_stats(ok) if ok.size else (float('nan'),) * 3) +
                  ("  undefined %d" % (il.size - ok.size) if ok.size < il.size else ""))
        if gain:
            print("depth gain median/mean/std: %.3f / %.3f / %.3f" % _stats(gain))
    except Exception as e:          # noqa: BLE001 - a command-line tool: report and exit non-zero
        print(f"error: {type(e).__name__}: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
