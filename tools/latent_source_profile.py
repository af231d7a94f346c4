"""The latent sources side by side at the benchmark's shape (1024 sequences x 300 frames, cfg glamr_dynamic, full schedule): what
DESIGN.md 10 'Measured' and profiles/latent_source_* were made with.

    python tools/latent_source_profile.py time                    # ONE stream: period of the captured step, both sources alternating in one
                                                                  #   process, 8 samples of 10 replays each -> profiles/latent_source_step_period.json
    python tools/latent_source_profile.py pipeline                # TWO gated streams (the pipeline bench.py times): period per batch, both sources
                                                                  #   -> profiles/latent_source_pipeline_period.json
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/latent_source_profile.py trace philox      # (or torch)
    python tools/latent_source_profile.py summarise DIR/NAME_results.db philox
                                                                  # per-kernel sums of the trace's dispatch records
                                                                  #   -> profiles/latent_source_<source>_resident_step_kernel_stats.csv
A trace covers 9 steps: two warm-up steps, the capture, its check (a plain step and a replay) and 5 replays."""
import csv
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, T, CFG = 1024, 300, 'glamr_dynamic'
SOURCES = ('torch', 'philox')


def summarise(db_path, source):
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = list(db.execute('select name, count(*), sum(end - start), avg(end - start), min(end - start), max(end - start) from kernels group by name order by 3 desc'))
    total = sum(r[2] for r in rows)
    out = os.path.join(ROOT, 'profiles', 'latent_source_%s_resident_step_kernel_stats.csv' % source)
    with open(out, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['Name', 'Calls', 'TotalDurationNs', 'AverageNs', 'Percentage', 'MinNs', 'MaxNs'])
        for r in rows:
            w.writerow([r[0], r[1], r[2], round(r[3], 1), round(100 * r[2] / total, 4), r[4], r[5]])
    print(out)


def setup():
    import torch
    from oracle.port import build as ob
    from glamr_amd.utils import synth
    from glamr_amd.lib.models.smpl import SMPL
    from glamr_amd.models.prior_models import MotionTrajJointModel
    dev = torch.device('cuda:0')
    root = ob.ensure_synthetic_assets(os.path.join(tempfile.gettempdir(), 'glamr_profile_assets'))
    smpl = SMPL(os.path.join(root, 'data', 'body_models', 'smpl'), pose_type='body26fk', extra_regressor_path=os.path.join(root, 'data', 'J_regressor_extra.npy')).to(dev)
    mt = MotionTrajJointModel(None, dev, None, smpl=smpl, results_root=os.path.join(root, 'results'))
    md = synth.make_smpl_model()
    t0 = time.time()
    batches = [[synth.make_in_dict(seed=base + s, num_frames=T, num_persons=1, smpl_model=md) for s in range(S)] for base in (0, 5000)]
    print('inputs: %.1f s' % (time.time() - t0), flush=True)
    return dev, smpl, mt, batches


def new_model(dev, smpl, mt, source):
    from glamr_amd.global_recon.configs import get_config
    from glamr_amd.global_recon.models import model_dict
    model = model_dict['global_recon_model'](get_config(CFG), dev, None, smpl=smpl, mt_model=mt)
    model.latent_source, model.latent_seed = source, 4
    return model


def graphs_for(env, source, gated):
    """The captured step of `source`: one graph on one stream, or -- gated -- two batches on two streams under a PipelineGate."""
    import torch
    from glamr_amd.global_recon.models.global_recon_model import PipelineGate
    dev, smpl, mt, batches = env
    model = new_model(dev, smpl, mt, source)
    n = 2 if gated else 1
    streams = [torch.cuda.Stream(device=dev) for _ in range(n)]
    rins = [model.stage_inputs(b) for b in batches[:n]]
    torch.cuda.synchronize()
    if gated:
        model.pipeline_gate = PipelineGate()
    for st, r in zip(streams, rins):
        for _ in range(2):
            with torch.cuda.stream(st):
                model.optimize_resident(r)
            torch.cuda.synchronize()
    if gated:
        model.pipeline_gate.last = None
    graphs = [model.capture_resident(r, stream=st, check=True) for st, r in zip(streams, rins)]
    torch.cuda.synchronize()
    return model, graphs, streams


def period(graphs, streams, n):
    """ms per replayed step (per batch when two graphs alternate), device events around n replays of every graph."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for st in streams[1:]:
        st.wait_stream(streams[0])
    with torch.cuda.stream(streams[0]):
        a.record()
    for _ in range(n):
        for g in graphs:
            g.replay()
    for st in streams[1:]:
        streams[0].wait_stream(st)
    with torch.cuda.stream(streams[0]):
        b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (n * len(graphs))


def timing(gated):
    import numpy as np
    env = setup()
    g = {s: graphs_for(env, s, gated) for s in SOURCES}
    for s in SOURCES:
        period(g[s][1], g[s][2], 5)
    res = {s: [] for s in SOURCES}
    for rep in range(8):
        for s in (SOURCES if rep % 2 == 0 else SOURCES[::-1]):
            res[s].append(period(g[s][1], g[s][2], 10))
    out = {s: {'ms_per_step': [round(x, 3) for x in v], 'mean': round(float(np.mean(v)), 3), 'min': round(min(v), 3), 'max': round(max(v), 3),
               'std': round(float(np.std(v)), 3)} for s, v in res.items()}
    out['workload'] = '%s, %d sequences x %d frames, cfg %s, full schedule, captured step replayed 10 times per sample (per graph), 8 samples per source, alternating' % (
        'two gated streams, two batches, ms per batch' if gated else 'one stream', S, T, CFG)
    print(json.dumps(out))
    name = 'latent_source_pipeline_period.json' if gated else 'latent_source_step_period.json'
    with open(os.path.join(ROOT, 'profiles', name), 'w') as f:
        json.dump(out, f, indent=1)


def trace(source):
    import torch
    _, graphs, _ = graphs_for(setup(), source, False)
    for _ in range(5):
        graphs[0].replay()
    torch.cuda.synchronize()
    print('traced 5 replays under', source)


if __name__ == '__main__':
    mode = sys.argv[1]
    if mode == 'summarise':
        summarise(sys.argv[2], sys.argv[3])
    elif mode in ('time', 'pipeline'):
        timing(mode == 'pipeline')
    else:
        trace(sys.argv[2])
