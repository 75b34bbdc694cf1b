# The part cuts of the skewed layout (per mille of the index's windows): every setting ROUNDS times, the settings alternately; one
# line per run on standard output.
#   bash tools/skew_sweep.sh [rounds] [win_cut1=..,win_cut2=.. ...]      (on C3's 153 windows: 392/730 = 59/52/42, 393/733 = 60/52/41,
#   393/730 = 60/51/42, 399/733 = 61/51/41, 393/739 = 60/53/40, 392/733 = 59/53/41, 380/730 = 58/53/42, 399/739 = 61/52/40)
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
ROUNDS=${1:-3}; shift
SETTINGS=${*:-win_cut1=392,win_cut2=730 win_cut1=393,win_cut2=733 win_cut1=393,win_cut2=730 win_cut1=399,win_cut2=733 win_cut1=393,win_cut2=739 win_cut1=392,win_cut2=733 win_cut1=380,win_cut2=730 win_cut1=399,win_cut2=739}
for r in $(seq $ROUNDS); do for t in $SETTINGS; do
  timeout -k 10 200 python bench.py --tune $t 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read()); print('run $r', '$t', 'kernel_ms', d['roofline']['kernel_ms'], 'step', d['ms_per_step'])" || exit 1
done; done
