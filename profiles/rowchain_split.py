"""k_rowchain launches of a rocprofv3 --kernel-trace database, averaged by their position inside a step (16 per step at
workload B: 0..7 forward chains of layers 0..7, 8..15 backward chains of layers 7..0).  usage: rowchain_split.py <db> [per_step=16]"""
import sqlite3, sys
db = sqlite3.connect(sys.argv[1]); cur = db.cursor()
per = int(sys.argv[2]) if len(sys.argv) > 2 else 16
tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
kd = [t for t in tabs if t.startswith('rocpd_kernel_dispatch')][0]
ks = [t for t in tabs if t.startswith('rocpd_info_kernel_symbol')][0]
rows = list(cur.execute(f"select s.kernel_name, d.start, d.end from {kd} d join {ks} s on d.kernel_id = s.id order by d.start"))
ch = [(n, e - s) for n, s, e in rows if 'k_rowchain' in n or 'k_chainres' in n]
print('chain launches', len(ch), 'steps', len(ch) / per)
nst = len(ch) // per
ch = ch[len(ch) - per * nst:]
skip = min(8, nst // 2)      # leave the first steps (warm-up, capture) out
pos = [[] for _ in range(per)]
for i, (n, d) in enumerate(ch):
    if i // per >= skip: pos[i % per].append((n, d))
for p in range(per):
    ds = [d for _, d in pos[p]]
    print(f'pos {p:2d} n={len(ds):3d} avg={sum(ds)/len(ds)/1e3:7.2f} us min={min(ds)/1e3:7.2f} max={max(ds)/1e3:7.2f}  {pos[p][0][0][:70]}')
f = [d for p in range(1, 8) for _, d in pos[p]]; b = [d for p in range(8, 15) for _, d in pos[p]]
print(f'forward chains of layers 1..7: avg {sum(f)/len(f)/1e3:.2f} us ; backward chains of layers 7..1: avg {sum(b)/len(b)/1e3:.2f} us')
