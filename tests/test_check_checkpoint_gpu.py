"""GPU test of tools/check_checkpoint.py on a synthetic checkpoint directory (built the way test_predict_cli_end_to_end builds its own:
config.yaml with unresolved interpolations + models/best.ckpt + two PNG pairs): one run of the tool per checkpoint, in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import lama_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISONED = 'model.6.conv1.bn_l.weight'            # the second (last) resnet block of the two-block generator


def _checkpoint_dir(tmp_path, name, poison):
    import yaml
    cfg = O.small_config(ngf=16, n_blocks=2)
    sd = O.make_synthetic_state_dict(cfg, seed=5, calib_hw=32)
    if poison:
        sd[POISONED] = sd[POISONED] * 1e6
    raw = dict(training_model=dict(kind='default', concat_mask=True),
               generator=dict(kind='ffc_resnet', **{k: v for k, v in cfg.items() if not isinstance(v, dict)},
                              init_conv_kwargs=dict(ratio_gin=0, ratio_gout=0, enable_lfu=False),
                              downsample_conv_kwargs=dict(ratio_gin='${generator.init_conv_kwargs.ratio_gout}',
                                                          ratio_gout='${generator.downsample_conv_kwargs.ratio_gin}', enable_lfu=False),
                              resnet_conv_kwargs=dict(ratio_gin=0.75, ratio_gout='${generator.resnet_conv_kwargs.ratio_gin}', enable_lfu=False)))
    mdir = tmp_path / name
    os.makedirs(mdir / 'models')
    with open(mdir / 'config.yaml', 'w') as f:
        yaml.safe_dump(raw, f)
    torch.save({'state_dict': {**{'generator.' + k: v for k, v in sd.items()}, 'discriminator.x': torch.zeros(2)}}, mdir / 'models' / 'best.ckpt')
    return mdir


@pytest.fixture(scope='module')
def indir(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp('in')
    rng = np.random.RandomState(3)
    for i, (h, w) in enumerate([(100, 136), (128, 128)]):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype('uint8')).save(d / f'im{i}.png')
        m = np.zeros((h, w), 'uint8')
        m[h // 3: 2 * h // 3, w // 4: w // 2] = 255
        Image.fromarray(m).save(d / f'im{i}_mask001.png')
    return d


def _run(mdir, indir, out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'check_checkpoint.py'), f'model.path={mdir}', f'indir={indir}', f'out={out}', *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_clean_checkpoint(tmp_path, indir):
    out = tmp_path / 'report.json'
    r = _run(_checkpoint_dir(tmp_path, 'clean', False), indir, out, 'oracle=true')
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    assert len(rep['images']) == 2 and rep['summary']['exit_status'] == 0 and rep['summary']['first_over'] is None
    for rec in rep['images']:
        names = [row['name'] for row in rec['rows']]
        assert names[0] == 'in' and 'model.6.conv2.ffc.convg2g.fu:spectrum' in names and names[-1] == 'model.19'
        assert all(row['n_over'] + row['n_nan'] + row['n_inf'] == 0 and not row['refused'] for row in rec['rows'])
        assert rec['watch_raised'] is False and rec['pack_refused'] is False and rec['range_error'] is None and rec['first_over'] is None
        assert set(rec['diff']) == {'f16x3_vs_bf16x3', 'f16x3_vs_f32', 'bf16x3_vs_f32'}
        print(rec['image'], rec['diff'], rec['oracle'])
        assert rec['diff']['f16x3_vs_f32']['max_abs'] < 1e-3                # the project's bar on `inpainted`
        assert all(d['max_abs'] < 1e-3 and d['u8_levels_differ'] >= 0 for d in rec['diff'].values())
        assert all(v < 1e-3 for v in rec['oracle'].values())
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(('f16x3:', 'bf16x3:', 'f32:'))]
    assert len(lines) == 3 and 'in range' in lines[0], r.stdout[-2000:]
    assert _run(tmp_path / 'clean', indir, out, 'bogus=1').returncode == 2   # a usage error: no GPU work
    open(tmp_path / 'clean' / 'models' / 'broken.ckpt', 'wb').write(b'not a checkpoint')
    assert _run(tmp_path / 'clean', indir, out, 'model.checkpoint=broken.ckpt').returncode == 3      # a failure is not a verdict


def test_poisoned_checkpoint_names_the_layer(tmp_path, indir):
    out = tmp_path / 'report.json'
    r = _run(_checkpoint_dir(tmp_path, 'poisoned', True), indir, out, 'n=1')
    assert r.returncode == 1, r.stdout[-3000:] + r.stderr[-3000:]
    verdict = [ln for ln in r.stdout.splitlines() if ln.startswith('f16x3:')]
    assert len(verdict) == 1 and 'OUT OF RANGE' in verdict[0] and 'model.6.conv1' in verdict[0], r.stdout[-2000:]
    rep = json.load(open(out))
    assert len(rep['images']) == 1 and rep['summary']['exit_status'] == 1
    rec = rep['images'][0]
    # the f16x3 forward ended with LamaRangeError: the watch raised in a launch, or the poisoned weight was refused when it was packed
    assert rec['first_over']['name'].startswith('model.6.conv1') and rec['watch_raised'] != rec['pack_refused'] and rec['range_error']
    print(rec['first_over'], rec['watch_raised'], rec['pack_refused'])
    bad = [row['name'] for row in rec['rows'] if row['n_over'] + row['n_nan'] + row['n_inf'] or row['refused']]
    assert bad[0].startswith('model.6.conv1'), bad                      # nothing in front of the poisoned layer is out of range
    assert rec['diff']['bf16x3_vs_f32'] is not None and rec['diff']['f16x3_vs_f32'] is None
