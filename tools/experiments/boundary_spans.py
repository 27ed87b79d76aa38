"""Workgroup spans of the headline's two raster kernels -- first workgroup's first stamp to last workgroup's last -- for setting
against their durations under rocprofv3 (boundary_trace.py): what a kernel costs outside its workgroups' lifetimes.
    python tools/experiments/boundary_spans.py bin      level 1 (PCA_BEV_DBG=32), per call: n_pend, write-back, span, pass B
    python tools/experiments/boundary_spans.py cells    the tile kernel (PCA_BEV_DBG=16), per call: span, mean lifetime
Numbers: profiles/bev_boundary_writethrough.txt."""
import sys, os, ctypes as C
which = sys.argv[1] if len(sys.argv) > 1 else 'bin'
os.environ['PCA_BEV_DBG'] = '32' if which == 'bin' else '16'
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'pc-accumulation-lib_amd'))
import numpy as np, builtins, bench, torch
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
out = {}
for rep in range(16):
    st.step(o)
    torch.cuda.synchronize()
    lib.pca_debug_bev_stamps(buf)
    a = np.array(buf[:]).reshape(1024, 8).astype(np.int64)
    if which == 'bin':
        tag = a[40, 6]                                        # (a window piece: the K1 tiles in front leave no stamps)
        h = a[(a[:, 0] > 0) & (a[:, 5] >= a[:, 0]) & (a[:, 6] == tag)]
        t0 = h[:, 0].min()
        h = h[(h[:, 0] - t0) < 20000]                         # this call's workgroups (stamps within 200 us of the first)
        ph = np.diff(h[:, :6], axis=1) / 100.0
        out.setdefault('n_pend %d write-back %d' % (tag // 2, tag % 2), []).append(
            (len(h), (h[:, 5].max() - t0) / 100.0, ph[:, 3].mean(), ph[:, 3].max(), ph[:, 0].mean(), ph[:, 2].mean()))
    else:
        h = a[a[:, 2] > 0]
        t0 = h[:, 0].min()
        out.setdefault('tile kernel', []).append((len(h), (h[:, 1].max() - t0) / 100.0, ((h[:, 1] - h[:, 0]) / 100.0).mean(), ((h[:, 1] - h[:, 0]) / 100.0).max(), 0., 0.))
builtins.print = rp
for k, v in sorted(out.items()):
    v = np.array(v)
    cols = 'workgroups, span us, pass B (registers) mean / max us, pass A mean us, scan mean us' if which == 'bin' else 'tiles, span us, lifetime mean / max us'
    print('%-28s calls %2d | %s | mean %s | span min %.1f max %.1f' % (k, len(v), cols, np.round(v.mean(0), 2).tolist()[:6 if which == 'bin' else 4], v[:, 1].min(), v[:, 1].max()))
