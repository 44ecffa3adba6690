"""The process tests/test_evaluate_gpu.py starts once for its end-to-end tests: ``python evaluate_child.py <dir>``.

It runs the CLI (``lama_amd.evaluate.main``) on the recorded dataset of tests/golden/evaluate.npz, the same run through ``build_evaluator`` and
``score_dataset`` with a tap on every batch, the direct SSIM / PerceptualLoss calls on the tapped tensors, ``InpaintingEvaluator.evaluate`` at
another batch size and the captured ingest launch, and pickles what it saw to ``<dir>/child.pkl`` as numpy arrays and plain Python objects.  It asserts nothing: every
assertion is in the test file.  A process of its own because the run captures hipGraphs, warms up on side streams and pins host memory: state a
test process keeps for good, and the plans other test files time against each other are sensitive to it ("how stable it is")."""
import os
import pickle
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import evaluate_ref as ER  # noqa: E402
import lpips_util as U  # noqa: E402
from lama_amd import _lib as L  # noqa: E402
from lama_amd import evaluate as EVL  # noqa: E402
from lama_amd import evaluation as EV  # noqa: E402


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().copy()


def _plain(results: dict) -> list:
    return [(k, {st: float(v) for st, v in d.items()}) for k, d in results.items()]


def end_to_end(root: str) -> dict:
    gold, lpips_gold = ER.load_gold(), np.load(U.GOLDEN)
    datadir, preddir = ER.write_dataset(gold, root)
    heads, backbone = os.path.join(root, 'heads.pth'), os.path.join(root, 'vgg16_seeded.pth')
    torch.save(U.heads_state_dict(lpips_gold), heads)
    torch.save(U.backbone_state_dict(), backbone)
    cfg = os.path.join(root, 'eval2.yaml')
    with open(cfg, 'w') as f:
        f.write('evaluator_kwargs:\n  batch_size: 8\n  device: cuda\n\ndataset_kwargs:\n'
                f'  img_suffix: {ER.IMG_SUFFIX}\n  inpainted_suffix: {ER.INPAINTED_SUFFIX}\n  pad_out_to_modulo: {ER.PAD_MOD}\n')
    out = os.path.join(root, 'out', 'report.tsv')
    rc = EVL.main([cfg, datadir, preddir, out, f'model_path={heads}', f'backbone={backbone}', 'io_threads=4'])
    taps = []
    ev = EVL.build_evaluator(EVL.load_config(cfg), datadir, preddir, model_path=heads, backbone=backbone)
    groups, names = EVL.score_dataset(ev.dataset, ev.scores, batch_size=ev.batch_size, device=ev.device, evaluator=ev, io_threads=4,
                                      clamp_image_range=ev.clamp_image_range,
                                      tap=lambda idx, image, pred, values, sums: taps.append((list(idx), image.clone(), pred.clone(),
                                                                                              {k: v.clone() for k, v in values.items()})))
    results = ev.results_of(groups, names)
    ssim_only = os.path.join(root, 'out', 'ssim_only.tsv')
    rc_ssim = EVL.main([cfg, datadir, preddir, ssim_only])
    ssim, lpips = ev.scores['ssim'].score, ev.scores['lpips'].score
    seen = []
    for idx, image, pred, values in taps:                    # the direct calls on the tensors the ingest launch left
        seen.append(dict(idx=idx, image=_np(image), pred=_np(pred), values={k: _np(v) for k, v in values.items()},
                         direct=dict(ssim=_np(ssim(pred, image)), lpips=_np(lpips(pred, image).flatten()))))
    other = EV.InpaintingEvaluator(ev.dataset, {'ssim': EV.SSIMScore()}, batch_size=5, device='cuda')
    return dict(rc=rc, rc_ssim=rc_ssim, report=open(out).read(), ssim_only=open(ssim_only).read(), results=_plain(results), taps=seen,
                groups=np.asarray(groups), individual={k: np.asarray(s.individual_values) for k, s in ev.scores.items()},
                evaluator_class=_plain(other.evaluate()))


def captured_ingest() -> dict:
    slot, pad_mod, sizes, batch = ER.INGEST_CASES['mixed_13x21']
    gt, pred, mask = (torch.from_numpy(a).cuda() for a in ER.ingest_inputs(slot, sizes, batch, seed=11))
    lib = L.get_lib()
    outs = [torch.zeros(batch, 3, 16, 24, device='cuda') for _ in range(4)]
    sums = [torch.zeros(batch, dtype=torch.int64, device='cuda') for _ in range(2)]
    lib.eval_ingest_u8(gt, pred, mask, sizes, pad_mod, outs[0], outs[1], sums[0], batch, clamp=(0.1, 0.9), stream=L.LamaLib.stream_of(gt))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lib.eval_ingest_u8(gt, pred, mask, sizes, pad_mod, outs[2], outs[3], sums[1], batch, clamp=(0.1, 0.9), stream=L.LamaLib.stream_of(gt))
    for t in outs[2:] + sums[1:]:
        t.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    return dict(plain=[_np(t) for t in outs[:2] + sums[:1]], replayed=[_np(t) for t in outs[2:] + sums[1:]])


if __name__ == '__main__':
    root = sys.argv[1]
    seen = dict(graph=captured_ingest(), **end_to_end(root))
    with open(os.path.join(root, 'child.pkl'), 'wb') as f:
        pickle.dump(seen, f)
