#!/bin/bash
# bench.py of two built trees of this repository on one box, alternating runs (the protocol of the records that set a commit against its parent):
#   tools/ab_two_trees.sh <parent tree> [runs = 5] [bench.py arguments ...]        (run from the tree under test; both trees built: python __graft_entry__.py)
# e.g. git worktree add /tmp/parent HEAD~1 && (cd /tmp/parent && python __graft_entry__.py) && tools/ab_two_trees.sh /tmp/parent 5 --steps 300 --warmup 20
# Every run is a process of its own under its own time limit; the first failing run ends the script.  Prints one line per run and the verdict by the
# rule of the records: the slowest run of this tree against the fastest run of the parent.
set -o pipefail
parent=${1:?parent tree}; shift
runs=${1:-5}; [ $# -gt 0 ] && shift
[ $# -gt 0 ] || set -- --steps 300 --warmup 20
here=$PWD
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
for i in $(seq 1 "$runs"); do
  for which in parent this; do
    if [ $which = parent ]; then dir=$parent; else dir=$here; fi
    ( cd "$dir" && timeout -k 10 300 python3 bench.py --gpus 1 "$@" ) > "$tmp/${which}_$i.json" 2> "$tmp/${which}_$i.err" || { echo "$which run $i failed"; tail -5 "$tmp/${which}_$i.err"; exit 1; }
  done
done
python3 - "$tmp" "$runs" "$*" <<'EOF'
import json, sys
tmp, runs, args = sys.argv[1], int(sys.argv[2]), sys.argv[3]
def value(path):
    for line in open(path):
        if line.lstrip().startswith("{"):
            return json.loads(line)["value"]
    raise SystemExit("no result line in " + path)
res = {w: [value("%s/%s_%d.json" % (tmp, w, i)) for i in range(1, runs + 1)] for w in ("parent", "this")}
print("# python bench.py --gpus 1 " + args)
for w in ("parent", "this"):
    print("%-7s it/s: %s   ms/step: %s" % (w, " ".join("%.1f" % v for v in res[w]), " ".join("%.4f" % (1e3 / v) for v in res[w])))
p, t = res["parent"], res["this"]
print("slowest run of this tree against the fastest run of the parent: x%.3f; the parent's own spread: %.1f %%" % (min(t) / max(p), 100 * (max(p) / min(p) - 1)))
EOF
