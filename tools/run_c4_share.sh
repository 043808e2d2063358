set -o pipefail
O=${OUT_DIR:-bench_out}/c4ab; mkdir -p $O
for sh in 1 2 3 6 1; do
  timeout -k 10 300 python bench.py --full --config c4 --no-cpu-baseline --steps 8 --warmup 2 --dsm-share $sh > $O/share$sh.json 2> $O/share$sh.err || { tail -5 $O/share$sh.err; exit 1; }
  python3 -c "import json; d=json.load(open('$O/share$sh.json')); print('share $sh', d['value'], d.get('pcie_inclusive',{}).get('value') if isinstance(d.get('pcie_inclusive'),dict) else '')"
done
