"""CPU tests of the weight-gradient GEMMs (tests/atb_common.py) on the x86 simulator build: eqd_atb on every body of
k_atb - general, atb_fast, atb_fast_bf with fp32 and saved-bf16 Y -, fp32 and bf16, at the 64-row chunk edges, with
three and more chunks per workgroup, through the planner's launch splits and under EQD_ATB_WGS / EQD_ATB_XCD_ALIGN,
against float64; and the model's ride-along tails (EQD_ATB_TAIL) on against off, bit for bit.

The simulator runs the threads of a workgroup one after the other between barriers, so a missing barrier cannot show
here (tests/test_atb_gpu.py runs the same cases on the device); and it copies the tail's job descriptor from the kernel
argument itself, not from the kernarg segment at a computed offset (#ifdef EQD_HOSTSIM in k_atb)."""
import pytest
import torch

from equidock_public_amd import _lib
from tests import atb_common as ac

DEV = torch.device('cpu')
MEASURE = {}


@pytest.fixture(scope='module', autouse=True)
def simulator():
    from tests.hostsim import build as hs
    _lib.load_library_for_testing(hs.build())
    assert _lib.is_simulator()
    yield
    _lib.reload_tunables()
    print('\n' + ac.report(MEASURE))
    _lib.unload_for_testing()


EDGE = ac.edge_cases()
MANY = ac.many_unit_cases()
PLANNER = ac.planner_cases()


@pytest.mark.parametrize('case', EDGE, ids=[c['id'] for c in EDGE])
def test_atb_row_edges(case, monkeypatch):
    ac.apply_env(monkeypatch, {})
    ac.check_case(DEV, case, measure=MEASURE)


@pytest.mark.parametrize('case', MANY, ids=[c['id'] for c in MANY])
def test_atb_many_units(case, monkeypatch):
    """three and more chunks per workgroup, unequal walks, a ragged last chunk.  (Twice from the same buffers with equal
    bits: on the device for every case; here, where workgroups run one after the other anyway and a second run of a
    32-unit call costs 5 - 9 s, for the small ones.)"""
    ac.apply_env(monkeypatch, case.get('env', {}))
    ac.check_case(DEV, case, measure=MEASURE, twice='env' in case)


@pytest.mark.parametrize('case', PLANNER, ids=[c['id'] for c in PLANNER])
def test_atb_planner(case, monkeypatch):
    ac.apply_env(monkeypatch, {})
    ac.check_case(DEV, case, measure=MEASURE, twice=1 < len(case['jobs']) < 20)


def test_atb_contract_errors(monkeypatch):
    ac.apply_env(monkeypatch, {})
    ac.check_contract_errors(DEV)


@pytest.mark.parametrize('name,base,va,vb,bits', ac.AGREE, ids=[a[0] for a in ac.AGREE])
def test_atb_bodies_agree(name, base, va, vb, bits, monkeypatch):
    ac.apply_env(monkeypatch, {})
    ac.check_bodies_agree(DEV, name, base, va, vb, bits)


@pytest.mark.parametrize('name', list(ac.TAIL_CONFIGS))
def test_atb_tails_on_against_off(name, monkeypatch):
    ac.check_tails(DEV, monkeypatch, name)


def test_every_body_is_covered():
    """the case list reaches every body k_atb dispatches to, each at every row edge"""
    want = {f'general<{n},{m}>' for n in (4, 5) for m in ('fp32', 'bf16')} | {f'fast<{k}>' for k in ('plain', 'masked')} | \
        {f'fast_bf<{y},{k}>' for y in ('f32', 'ybf') for k in ('plain', 'masked')}
    seen = {}
    for case in EDGE:
        jobs, plan = ac.case_plan(case)
        for u in plan['units']:
            if u['nchunks']:
                seen.setdefault(u['body'], set()).add(jobs[0]['rows'])
    assert set(seen) == want, set(seen) ^ want
    for b, rows in seen.items():
        assert rows == set(ac.ROW_EDGES) - {0}, (b, sorted(rows))
    # the 2 GB fallback of atb_fast_bf is a host-side condition that is restated, not run
    big = ac.job(64, 64, 2 ** 23, bf16=1)
    assert ac.expected_plan(ac._keys(dict(jobs=[big])))['units'][0]['body'] == 'general<4,bf16>'
    assert ac.expected_plan(ac._keys(dict(jobs=[dict(big, rows=2 ** 23 - 1)])))['units'][0]['body'] == 'fast_bf<f32,plain>'


def test_float32_yardstick():
    """the bounds are 8 x (column sums 5 x) what is recorded in F32_MEASURED: re-measure the float32 evaluation of the
    reference over this file's cases and the GPU file's larger ones.  The evaluation has a fixed order of elementwise
    operations (atb_common.f32_product), so nothing may exceed the record - on any machine, at any thread count."""
    worst = ac.yardstick(ac.all_cases(gpu=True))
    for (mode, cls, big), e in sorted(worst.items()):
        rec = ac.F32_MEASURED[mode][cls]
        print(f"{mode} {cls} {'rows >= 4096' if big else ''}: float32 evaluation {e:.2e}, recorded {rec:.2e}")
        assert e <= rec, (mode, cls, big, e, rec)
