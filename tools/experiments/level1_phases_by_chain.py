"""Level 1's phases on the headline, from the PCA_BEV_DBG=32 stamps, averaged per kind of call (owed chain length, write-back):
mean over the store's workgroups and over `reps` steps, us per workgroup.
    python tools/experiments/level1_phases_by_chain.py [reps] [label]
Numbers: profiles/bev_level1_lds_overflow.txt."""
import ctypes as C
import os
import sys
os.environ['PCA_BEV_DBG'] = '32'
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'pc-accumulation-lib_amd'))
import builtins
import numpy as np
import bench
import torch
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
label = sys.argv[2] if len(sys.argv) > 2 else ''
rp = builtins.print
builtins.print = lambda *a, **k: None
acc, pool, _ = bench.make_accumulator(bench.synth_frame, 0)
st = bench.Stepper(acc, pool)
st.fill()
o = torch.empty((21, bench.PX, bench.PX), dtype=torch.float16, device='cuda')
for _ in range(40):
    st.step(o)
from pca_amd import _lib
lib = _lib.Context.get().lib
buf = (C.c_ulonglong * 8192)()
names = ['setup + pass A resident', 'pass A memory + barrier', 'scan', 'pass B resident', 'pass B memory']
acc_ph, acc_span, acc_n = {}, {}, {}
for rep in range(reps):
    st.step(o)
    torch.cuda.synchronize()
    lib.pca_debug_bev_stamps(buf)
    a = np.array(buf[:]).reshape(1024, 8).astype(np.int64)
    tag = a[30, 6]
    live = (a[:, 0] > 0) & (a[:, 5] >= a[:, 0]) & (a[:, 6] == tag)
    h = a[live]
    if len(h) == 0:
        continue
    t0 = h[:, 0].min()
    fresh = h[(h[:, 0] - t0) < 20000]                       # this call's workgroups (stamps within 200 us of the first)
    ph = np.diff(fresh[:, :6], axis=1) / 100.0
    key = (int(tag // 2), int(tag % 2), len(fresh))
    acc_ph.setdefault(key, []).append(ph.mean(axis=0))
    acc_span.setdefault(key, []).append((fresh[:, 5].max() - t0) / 100.0)
    acc_n[key] = acc_n.get(key, 0) + 1
builtins.print = rp
for key in sorted(acc_ph):
    ph = np.mean(acc_ph[key], axis=0)
    print('%-8s n_pend %d wb %d workgroups %3d calls %2d | span %.1f | life %.1f | ' % (label, key[0], key[1], key[2], acc_n[key], np.mean(acc_span[key]), ph.sum())
          + ' | '.join('%s %.2f' % (n, ph[k]) for k, n in enumerate(names)))
