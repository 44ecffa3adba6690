"""Pin oracle/refine_oracle.py to the REFERENCE's own ``saicinpainting/evaluation/refinement.py:86-174,228-314``.

tests/golden/make_golden_refine_pin.py imported the reference module UNMODIFIED (with stubs for what it cannot import, each bound to a
helper pinned by known-answer vectors in tests/test_refine_helpers_known_answers.py), ran its ``refine_predict`` with the reference's
own ``FFCResNetGenerator`` (reference factory, state dict loaded with strict=True) and stored, per case, the shape, the SHA-256 of
the fp32 output bytes and a strided sample of it in golden/refine_pin.npz.
Here ``oracle.refine_oracle.refine_predict`` runs on the same seeded inputs and state dict.  Control flow, pyramid, masks, loss, Adam
and the final blend must agree BIT FOR BIT (both sides execute the same torch primitives in the same order, on one intra-op thread).
"""
import contextlib
import importlib.util
import os

import numpy as np
import pytest
import torch

_SPEC = importlib.util.spec_from_file_location(
    'make_golden_refine_pin', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'make_golden_refine_pin.py'))
MK = importlib.util.module_from_spec(_SPEC)
_SPEC.loader.exec_module(MK)
CASES = MK.CASES


@contextlib.contextmanager
def _one_thread():
    """As the golden run: the bits (of the BatchNorm calibration pass too) must not depend on the core count."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


@pytest.fixture(scope='module')
def pin(golden_dir):
    from oracle import lama_oracle as O
    cfg = MK.config()
    with _one_thread():
        sd = O.make_synthetic_state_dict(cfg, seed=MK.SEED_SD, calib_hw=32)
    return np.load(os.path.join(golden_dir, 'refine_pin.npz')), cfg, sd


@pytest.mark.parametrize('h,w,kw,gray', CASES)
def test_refine_oracle_equals_reference_refinement(pin, h, w, kw, gray):
    from oracle import refine_oracle as R
    g, cfg, sd = pin
    i = CASES.index((h, w, kw, gray))
    trace = []
    with _one_thread():
        image_p, mask_p = MK.make_case(h, w, gray)
        got = R.refine_predict(image_p.clone(), mask_p.clone(), (h, w), sd, cfg, modulo=8, n_iters=MK.N_ITERS, lr=MK.LR, trace=trace, **kw)
    assert len(trace) >= 2                                                            # the refinement loop ran, not only the plain forward
    assert all(len(t.get('loss', [])) == MK.N_ITERS for t in trace[1:])
    assert tuple(got.shape) == tuple(g[f'shape{i}'])
    got_sample, want_sample = MK.sample(got), g[f'sample{i}']
    assert np.array_equal(got_sample, want_sample), float(np.abs(got_sample - want_sample).max())
    assert np.array_equal(MK.digest(got), g[f'sha256_{i}']), 'the output differs from the reference outside the stored sample'
