"""Wall time of a MUTAG batch-of-32 training step (GNNgraphBased.training_step, Adam on the device, no Dropout in net_state, BatchNormalization
behind it: every step runs max_iteration bodies) with 10 and with 50 bodies, and of a control the persistent training forward cannot
touch - a 4,096-row node-based step, which takes the matrix-core forms: warm, then the median over repeated steps (every step ends in the
step's wait for the device).  One JSON line.  --package DIR measures another build of the package (a folder that holds GNN/ with its
libgnn_hip.so) on the same data, e.g. the parent commit's, so that two trees can be run in turns on one machine; --persistent 0 keeps this
build to one launch per kernel and body (ignored by a build without the switch):
    python tools/bench_train_persistent.py [--package DIR] [--steps 200] [--persistent 1] [--tag NAME]"""
import argparse, json, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--package', default=None)
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--persistent', type=int, default=1)
ap.add_argument('--tag', default='this')
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(args.package) if args.package else os.path.join(ROOT, 'gnn_tf_2.x_amd')
sys.path.insert(0, PKG)
from GNN import losses, optimizers
from GNN.GNN import GNNgraphBased, GNNnodeBased
from GNN.MLP import MLP, set_seed
from GNN.graph_class import GraphObject, GraphTensor
import load_MUTAG
load_MUTAG._PACKED = os.path.join(ROOT, 'tests', 'golden', 'mutag_raw.npz')

graphs = load_MUTAG.load(limit=128)
batches = [GraphTensor.fromGraphObject(GraphObject.merge(graphs[i:i + 32], problem_based='g', aggregation_mode='average')) for i in range(0, 128, 32)]
forms = []


def with_form(gnn):
    inner = gnn._device_loop

    def device_loop(dev_graph):
        loop = inner(dev_graph)
        if hasattr(loop, 'set_train_persistent') and getattr(loop, '_tp_set', None) != args.persistent:
            loop.set_train_persistent(bool(args.persistent))
            loop._tp_set = args.persistent
        forms.append(loop)
        return loop

    gnn._device_loop = device_loop
    return gnn


def mutag_model(bodies):
    set_seed(0)
    st = MLP(3 + 2 * 14, [32, 32, 14], 'selu', 'glorot_normal', 'zeros')
    ou = MLP(14, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    return with_form(GNNgraphBased(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.001), loss_function=losses.categorical_crossentropy, loss_arguments=None,
                                   state_vect_dim=0, max_iteration=bodies, threshold=0.001, addressed_problem='c'))


def control():
    rng = np.random.default_rng(0)
    n = 4096
    src = rng.integers(0, n, 3 * n); dst = (src + 1 + rng.integers(0, n - 1, 3 * n)) % n
    und = np.unique(np.stack([np.minimum(src, dst), np.maximum(src, dst)], 1), axis=0)
    ids = np.concatenate([und, und[:, ::-1]])
    arcs = np.concatenate([ids.astype(np.float32), (2 * rng.random((len(ids), 1)) - 1).astype(np.float32)], axis=1)
    arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))]
    nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
    go = GraphObject(arcs=arcs, nodes=nodes, targets=np.eye(2)[rng.integers(0, 2, n)], problem_based='n', aggregation_mode='average')
    set_seed(0)
    st = MLP(1 + 2 * 3, [32, 32, 3], 'selu', 'glorot_normal', 'zeros')
    ou = MLP(3, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    gnn = with_form(GNNnodeBased(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.001), loss_function=losses.categorical_crossentropy, loss_arguments=None,
                                 state_vect_dim=0, max_iteration=10, threshold=0.001, addressed_problem='c'))
    return gnn, [GraphTensor.fromGraphObject(go)]


def measure(gnn, data):
    for _ in range(5):
        for b in data: r = gnn.training_step(b, True)
    times = []
    for i in range(args.steps):
        t0 = time.perf_counter()
        r = gnn.training_step(data[i % len(data)], True)
        times.append(time.perf_counter() - t0)
    t = 1e3 * np.sort(times)
    info = forms[-1].train_info() if forms and hasattr(forms[-1], 'train_info') else {}
    return dict(median_ms=round(float(np.median(t)), 4), p10_ms=round(float(t[len(t) // 10]), 4), p90_ms=round(float(t[(9 * len(t)) // 10]), 4),
                k=r['k'], loss=round(float(r['loss']), 5), persistent=bool(info.get('persistent', False)), timeouts=int(info.get('timeouts', 0)))


out = dict(tag=args.tag, steps=args.steps)
out['mutag10'] = measure(mutag_model(10), batches)
out['mutag50'] = measure(mutag_model(50), batches)
out['control4096'] = measure(*control())
print(json.dumps(out), flush=True)
