"""GPU tests (-m gpu) of the node-update row chains (tests/node_chain_common.py) on a real MI355X: the simulator file's
cases - every kernel body of eqd_launch_rowchain, fp32 and bf16, at 16-row tile edges and k_rowres workgroup edges - and,
under the default switches, row counts derived from the device's CU count that walk the dispatch across tiles == CUs,
tiles == CUs + 1 and the 3 x CUs threshold of k_rowres, against float64."""
import pytest
import torch

from tests import node_chain_common as nc

pytestmark = pytest.mark.gpu
MEASURE = {}


@pytest.fixture(scope='module')
def dev():
    from equidock_public_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.unload_for_testing()
    _lib.load_library()
    assert not _lib.is_simulator()
    yield torch.device('cuda:0')
    print('\n' + nc.report(MEASURE))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(dev, monkeypatch, cases):
    for cid, body, bf16, cfg, rows, family, drop in cases:
        nc.apply_env(monkeypatch, nc.BODIES[body])
        nc.check_case(dev, nc.make_case(nc.CONFIGS[cfg], rows, family, drop), bf16, nc.BODIES[body], _cus(), measure=MEASURE)


@pytest.mark.parametrize('body', list(nc.BODIES))
def test_node_chain_row_edges(dev, body, monkeypatch):
    _run(dev, monkeypatch, nc.thinned_cases((body,)))


def test_node_chain_rowres_workgroup_edges(dev, monkeypatch):
    _run(dev, monkeypatch, nc.rowres_cases())


def test_node_chain_default_dispatch_sizes(dev, monkeypatch):
    """4096, 4097, 4112, 12272, 12288, 12289 rows on a 256-CU device, and 40000: k_rowchain_res_fwd / <1, ., 1> up to one
    tile per CU, <1, ., 2> past it, k_rowres (k_rowres80) from three tiles per CU"""
    cus = _cus()
    cases = nc.big_cases(cus)
    bodies = {nc.expected_bodies({}, nc.CONFIGS[c[3]], c[2], c[4], cus)[0][1] for c in cases}
    assert {'k_rowchain<1,1>', 'k_rowchain<1,2>', 'k_rowres', 'k_rowres80', 'k_rowchain_res_fwd'} <= bodies, bodies
    _run(dev, monkeypatch, cases)


def test_gradients_accumulate(dev, monkeypatch):
    for body, bf16, cfg in nc.TWICE:
        nc.apply_env(monkeypatch, nc.BODIES[body])
        nc.check_twice(dev, nc.make_case(nc.CONFIGS[cfg], 77, 'plain', True), bf16, nc.BODIES[body], _cus())


def test_bodies_agree(dev, monkeypatch):
    for bf16, cfg, rows, family, bodies in nc.AGREE:
        nc.check_bodies_agree(dev, monkeypatch, nc.make_case(nc.CONFIGS[cfg], rows, family, True), bf16, bodies, _cus())
