#!/bin/bash
# Part (d) of profiles/r20_keyset_remove.jsonl on ONE box: jjs_keyset_verify_dev on a set that was never removed from
# (tools/keyset_remove_rate.py --only d) and bench.py, in this tree and in a checkout of the parent commit, processes alternating,
# the order within a pair swapped from pair to pair (this-parent, parent-this, ...).  The parent tree is built and holds a copy of
# tools/keyset_remove_rate.py.
# Usage: bash scripts/keyset_remove_ab.sh /path/to/parent-tree [pairs] [out.jsonl] [bench steps] [bench warmup]      (rows are appended
# to out.jsonl; RATE=0 in the environment: the bench.py pairs alone)
set -o pipefail
P=${1:?the tree of the parent commit}; N=${2:-4}; HERE=$PWD; OUT=${3:-$HERE/profiles/r20_keyset_remove.jsonl}; STEPS=${4:-20}; WARM=${5:-5}
case $P in /*) ;; *) P=$HERE/$P;; esac
case $OUT in /*) ;; *) OUT=$HERE/$OUT;; esac
rate() {
  (cd "$1" && timeout -k 10 120 python jubjub_schnorr_amd/tools/keyset_remove_rate.py --only d --tree "$2" --process "$3" --out "$OUT" > /dev/null) || exit 1
}
step() {
  (cd "$1" && timeout -k 10 300 python bench.py --gpus 1 --steps "$STEPS" --warmup "$WARM" 2>/dev/null | tail -1 | python -c 'import sys, json; print(json.loads(sys.stdin.read())["ms_per_step"])') || exit 1
}
for i in $(seq "$([ "${RATE:-1}" = 0 ] && echo 0 || echo "$N")"); do
  if [ $((i % 2)) = 1 ]; then rate "$HERE" this "$i"; rate "$P" parent "$i"; else rate "$P" parent "$i"; rate "$HERE" this "$i"; fi
done
for i in $(seq "$N"); do
  if [ $((i % 2)) = 1 ]; then a=$(step "$HERE") && b=$(step "$P") || exit 1; first=this; else b=$(step "$P") && a=$(step "$HERE") || exit 1; first=parent; fi
  python -c 'import sys, json; print(json.dumps({"part": "d", "what": "bench.py --gpus 1 --steps %s --warmup %s, ms_per_step" % (sys.argv[5], sys.argv[6]), "pair": int(sys.argv[1]), "first": sys.argv[2], "this": round(float(sys.argv[3]), 4), "parent": round(float(sys.argv[4]), 4)}))' "$i" "$first" "$a" "$b" "$STEPS" "$WARM" | tee -a "$OUT"
done
