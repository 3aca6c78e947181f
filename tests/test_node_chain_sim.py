"""CPU tests of the node-update row chains (tests/node_chain_common.py) on the x86 simulator build: eqd_node_update_fwd /
_bwd under every kernel body of eqd_launch_rowchain, fp32 and bf16, at 16-row tile edges and at k_rowres workgroup edges,
against float64.  The full cross product (11 width configurations x 3 input families x dropout on / off x 12 switch
sets x 2 modes x 11 row edges) is thinned: every body runs every row edge in both modes, and the configuration, the
input family and dropout rotate along the row edges (node_chain_common.thinned_cases)."""
import pytest
import torch

from equidock_public_amd import _lib
from tests import node_chain_common as nc

DEV = torch.device('cpu')
CUS = 256      # the simulated device (tests/hostsim/hip/hip_runtime.h)
MEASURE = {}


@pytest.fixture(scope='module', autouse=True)
def simulator():
    from tests.hostsim import build as hs
    _lib.load_library_for_testing(hs.build())
    assert _lib.is_simulator()
    yield
    print('\n' + nc.report(MEASURE))
    _lib.unload_for_testing()


CASES = nc.thinned_cases() + nc.rowres_cases()


@pytest.mark.parametrize('body,bf16,cfg,rows,family,drop', [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_node_chain(body, bf16, cfg, rows, family, drop, monkeypatch):
    nc.apply_env(monkeypatch, nc.BODIES[body])
    nc.check_case(DEV, nc.make_case(nc.CONFIGS[cfg], rows, family, drop), bf16, nc.BODIES[body], CUS, measure=MEASURE)


@pytest.mark.parametrize('body,bf16,cfg', nc.TWICE, ids=[f"{b}-{'bf16' if m else 'fp32'}-{c}" for b, m, c in nc.TWICE])
def test_gradients_accumulate(body, bf16, cfg, monkeypatch):
    """two backward calls into the same buffers: exactly twice one call's parameter gradients, for one case per body"""
    nc.apply_env(monkeypatch, nc.BODIES[body])
    nc.check_twice(DEV, nc.make_case(nc.CONFIGS[cfg], 77, 'plain', True), bf16, nc.BODIES[body], CUS)


@pytest.mark.parametrize('bf16,cfg,rows,family,bodies', nc.AGREE,
                         ids=[f"{'bf16' if m else 'fp32'}-{c}-r{r}-{f}" for m, c, r, f, _ in nc.AGREE])
def test_bodies_agree(bf16, cfg, rows, family, bodies, monkeypatch):
    nc.check_bodies_agree(DEV, monkeypatch, nc.make_case(nc.CONFIGS[cfg], rows, family, True), bf16, bodies, CUS)


def test_reference_is_autograd():
    """the hand-written float64 forward and backward of node_reference equal float64 autograd of the formula as written"""
    for cfg in nc.CONFIGS.values():
        for drop in (False, True):
            case = nc.make_case(cfg, 37, 'plain', drop)
            ref, auto = nc.node_reference(case, 0), nc.autograd_reference(case)
            for k, a in auto.items():
                if a is not None:
                    assert nc.rel_max(ref[k], a) <= 1e-13, (cfg['id'], drop, k, nc.rel_max(ref[k], a))


def test_float32_yardstick():
    """the bounds are 8 x what is recorded in F32_MEASURED / F32_FLIP: re-measure the float32 evaluation of the reference
    over this file's cases and the GPU file's large ones.  Its summation order belongs to the torch build, so the check is
    that nothing measured is beyond 1.5 x its record (the bounds then still stand 5 x above the yardstick)."""
    worst = nc.yardstick(CASES + nc.big_cases(CUS))
    for (mode, fam, cls, _), e in sorted(worst.items(), key=str):
        if cls == 'h_out:cap':
            assert e <= 1.0 or fam == 'shift', (mode, fam, cls, e)      # (the shift family: see FLIP_CAP_SCALE)
            continue
        if cls == 'dz' and mode == 'fp32':      # (only bf16 mode rounds dz: open_eps)
            continue
        rec = nc.F32_FLIP[fam] if cls == 'h_out:e2e' else nc.F32_MEASURED[mode, fam].get(cls)
        if rec is None:      # bf16 fwd / row_x / w_x: held to the fp32-mode bounds; the yardstick must sit below them / 8
            rec = nc.TOL[mode, fam][cls] / nc.FACTOR
        print(f'{mode} {fam} {cls}: float32 evaluation {e:.2e}, recorded {rec:.2e}')
        assert e <= 1.5 * rec, (mode, fam, cls, e, rec)


def test_expected_bodies_unreachable():
    """what the operator cannot reach, so that the coverage list is complete: fp32 d_in = 69 never leaves k_rowchain; the
    backward reaches k_rowwave / plain k_rowres only with d0 = 64; k_rowres80 needs bf16 and a 65..80-wide job"""
    for env in nc.BODIES.values():
        f, b = nc.expected_bodies(env, nc.CONFIGS['69x69'], 0, 33, CUS)
        assert f[0] == b[0] == 'k_rowchain'
        for cfg in nc.CONFIGS.values():
            for bf16 in (0, 1):
                f, b = nc.expected_bodies(env, cfg, bf16, 33, CUS)
                assert b[1] not in ('k_rowwave', 'k_rowres') or cfg['d0'] == 64
                assert 'k_rowres80' not in (f[1], b[1]) or (bf16 and max(cfg['d'], cfg['d0']) > 64)
                assert b[1] != 'k_rowchain_res_fwd' and (f[1] != 'k_rowchain_res_fwd' or not bf16)
