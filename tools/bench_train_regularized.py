"""Wall time of a MUTAG batch-of-32 training step (GNNgraphBased.training_step, 10 bodies, Adam) with l2(0.01) kernel regularizers on
both nets and, as the control, without any: warm, then the median over repeated steps (every step ends in the step's wait for the
device).  One JSON line.  --package DIR measures another build of the package (a folder that holds GNN/ with its libgnn_hip.so) on
the same data, e.g. the parent commit's, so that two trees can be run in turns on one machine:
    python tools/bench_train_regularized.py [--package DIR] [--steps 200] [--tag NAME]"""
import argparse, json, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--package', default=None)
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--tag', default='this')
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(args.package) if args.package else os.path.join(ROOT, 'gnn_tf_2.x_amd')
sys.path.insert(0, PKG)
from GNN import losses, optimizers, regularizers
from GNN.GNN import GNNgraphBased
from GNN.MLP import MLP, set_seed
from GNN.graph_class import GraphObject, GraphTensor
import load_MUTAG
load_MUTAG._PACKED = os.path.join(ROOT, 'tests', 'golden', 'mutag_raw.npz')

graphs = load_MUTAG.load(limit=128)
batches = [GraphTensor.fromGraphObject(GraphObject.merge(graphs[i:i + 32], problem_based='g', aggregation_mode='average')) for i in range(0, 128, 32)]


def model(reg):
    set_seed(0)
    st = MLP(3 + 2 * 14, [32, 32, 14], 'selu', 'glorot_normal', 'zeros', kernel_regularizer=reg, dropout_rate=0.1, dropout_pos=0)
    ou = MLP(14, [2], 'softmax', 'glorot_normal', 'zeros', kernel_regularizer=reg, batch_normalization=False)
    return GNNgraphBased(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.001), loss_function=losses.categorical_crossentropy, loss_arguments=None,
                         state_vect_dim=0, max_iteration=10, threshold=0.001, addressed_problem='c')


def measure(gnn):
    for _ in range(5):
        for b in batches: r = gnn.training_step(b, True)
    times = []
    for i in range(args.steps):
        t0 = time.perf_counter()
        r = gnn.training_step(batches[i % len(batches)], True)
        times.append(time.perf_counter() - t0)
    t = 1e3 * np.sort(times)
    return dict(median_ms=round(float(np.median(t)), 4), p10_ms=round(float(t[len(t) // 10]), 4), p90_ms=round(float(t[(9 * len(t)) // 10]), 4),
                k=r['k'], loss=round(float(r['loss']), 5), on_device=bool(gnn.net_state._host_stale))


out = dict(tag=args.tag, steps=args.steps)
plain, reg = model(None), model(regularizers.l2(0.01))
out['plain'] = measure(plain)
out['l2_kernels'] = measure(reg)
print(json.dumps(out), flush=True)
