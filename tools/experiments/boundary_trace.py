"""Reads the kernel trace of a `rocprofv3 --kernel-trace --output-format csv` run of bench.py and prints, for level 1 and the
tile kernel of the headline, hinted one-round calls and write-back calls apart: mean duration, and the mean gap between
level 1's end and the tile kernel's start and between the tile kernel's end and the next kernel's start.
    python tools/experiments/boundary_trace.py <dir given to rocprofv3 -d> [label]
Numbers: profiles/bev_boundary_writethrough.txt."""
import csv, glob, sys
import numpy as np
rows = []
for f in glob.glob(sys.argv[1] + '/**/*kernel_trace.csv', recursive=True):
    for r in csv.DictReader(open(f)):
        gx = r.get('Grid_Size_X') or r.get('Grid_Size') or '0'
        rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'], int(gx)))
rows.sort()
bins = [i for i, r in enumerate(rows) if r[2].startswith('bev_tile_bin_k1')]
bins = bins[len(bins) // 4:]                                  # steady state
grids = sorted({rows[i][3] for i in bins})
label = sys.argv[2] if len(sys.argv) > 2 else ''
for g in grids:
    sel = [i for i in bins if rows[i][3] == g and i + 2 < len(rows) and 'bev_tile_cells' in rows[i + 1][2]]
    if len(sel) < 5:
        continue
    b = np.array([rows[i][1] - rows[i][0] for i in sel]) / 1e3
    c = np.array([rows[i + 1][1] - rows[i + 1][0] for i in sel]) / 1e3
    g1 = np.array([rows[i + 1][0] - rows[i][1] for i in sel]) / 1e3
    g2 = np.array([rows[i + 2][0] - rows[i + 1][1] for i in sel]) / 1e3
    kind = 'hinted one-round' if g == grids[0] and len(grids) > 1 else 'write-back / full'
    print('%-8s %-18s grid %7d calls %4d | level 1 %.2f (median %.2f) | tile kernel %.2f (median %.2f) | gap level 1 -> tile kernel %.2f (median %.2f) | tile kernel -> next %.2f (median %.2f) us'
          % (label, kind, g, len(sel), b.mean(), np.median(b), c.mean(), np.median(c), g1.mean(), np.median(g1), g2.mean(), np.median(g2)))
