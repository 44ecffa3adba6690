"""The process tests/test_fid_gpu.py starts once for its graph and end-to-end tests: ``python fid_child.py <dir>``.

It replays the captured InceptionV3 launch sequence beside the eager one, runs the CLI (``lama_amd.evaluate.main``) on the recorded dataset of
tests/golden/evaluate.npz with LPIPS and ``fid_weights=``, the same run through ``evaluate_predicts`` with a tap on every batch, InceptionV3
directly on the tapped tensors, and the CLI without ``fid_weights=``, and pickles what it saw to ``<dir>/child.pkl`` as numpy arrays and plain
Python objects.  It asserts nothing: every assertion is in the test file.  A process of its own for the reason tests/evaluate_child.py gives: the
run captures hipGraphs, warms up on side streams and pins host memory -- state a test process keeps for good, and the plans other test files time
against each other are sensitive to it ("how stable it is")."""
import contextlib
import io
import os
import pickle
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import evaluate_ref as ER  # noqa: E402
import inception_util as U  # noqa: E402
import lpips_util as LU  # noqa: E402
from lama_amd import evaluate as EVL  # noqa: E402
from lama_amd import evaluation as EV  # noqa: E402


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().copy()


def graph_replay(gold, weights) -> dict:
    pred, target = (t.cuda() for t in U.case_inputs(gold, 'a'))
    eager = EV.InceptionV3([3], weights=weights).cuda()
    graphed = EV.InceptionV3([3], weights=weights).cuda()
    graphed.use_graph = True
    out = dict(eager=_np(torch.cat(eager.pair(pred, target))))
    out['capture'] = _np(torch.cat(graphed.pair(pred, target)))
    out['replay'] = _np(torch.cat(graphed.pair(pred, target)))
    out['swapped'] = _np(torch.cat(graphed.pair(target, pred)))          # other inputs through the same graph
    out['captured'] = all(p['graph'] is not None for p in graphed._plans.values()) and len(graphed._plans) == 1
    return out


def end_to_end(root: str, weights) -> dict:
    gold = ER.load_gold()
    datadir, preddir = ER.write_dataset(gold, root)
    paths = {k: os.path.join(root, k + '.pth') for k in ('inception', 'heads', 'vgg16')}
    torch.save(weights, paths['inception'])
    torch.save(LU.heads_state_dict(np.load(LU.GOLDEN)), paths['heads'])
    torch.save(LU.backbone_state_dict(), paths['vgg16'])
    cfg = os.path.join(root, 'eval.yaml')
    with open(cfg, 'w') as f:
        f.write('evaluator_kwargs:\n  batch_size: 8\n  device: cuda\ndataset_kwargs:\n  img_suffix: .png\n  inpainted_suffix: _inpainted.png\n'
                f'  pad_out_to_modulo: {ER.PAD_MOD}\n')
    seen = {}
    opts = [f'model_path={paths["heads"]}', f'backbone={paths["vgg16"]}', f'fid_weights={paths["inception"]}']
    with contextlib.redirect_stdout(io.StringIO()):
        seen['rc'] = EVL.main([cfg, datadir, preddir, os.path.join(root, 'report.tsv')] + opts)
    seen['report'] = open(os.path.join(root, 'report.tsv')).read()
    taps = []
    results = EVL.evaluate_predicts(EVL.load_config(cfg), datadir, preddir, None, fid_weights=paths['inception'], log=lambda *a: None,
                                    tap=lambda idx, image, pred, values, sums: taps.append((list(idx), image.clone(), pred.clone())))
    seen['results'] = [(k, {st: float(v) for st, v in d.items()}) for k, d in results.items()]
    model = EV.InceptionV3([3], weights=weights).cuda()
    n = len(ER.item_names(gold))
    ap, at = np.zeros((n, 2048), np.float32), np.zeros((n, 2048), np.float32)
    for idx, image, pred in taps:
        p, t = model.pair(pred, image)
        ap[idx], at[idx] = _np(p.flatten(1)), _np(t.flatten(1))
    seen['direct_pred'], seen['direct_target'] = ap, at
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        seen['rc_plain'] = EVL.main([cfg, datadir, preddir, os.path.join(root, 'plain.tsv')])
    seen['plain_stdout'], seen['plain_report'] = buf.getvalue(), open(os.path.join(root, 'plain.tsv')).read()
    return seen


if __name__ == '__main__':
    root = sys.argv[1]
    gold = np.load(U.GOLDEN)
    weights = U.synthetic_state_dict(gold)
    seen = dict(graph=graph_replay(gold, weights))
    seen.update(end_to_end(root, weights))
    torch.cuda.synchronize()
    with open(os.path.join(root, 'child.pkl'), 'wb') as f:
        pickle.dump(seen, f)
