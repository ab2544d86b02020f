cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
timeout 1500 python -m pytest tests -m gpu -x -q > gpurun_out/r6_full_tests.log 2>&1; tail -4 gpurun_out/r6_full_tests.log
timeout 900 python bench.py --full | tail -1 | python -c "
import json, sys
d = json.loads(sys.stdin.read())
print(d['value'], d['ms_per_step'], d['roofline']['frac'], d.get('fp32_exact'), d['crnn']['value'], d['crnn']['ms_per_step'], d['crnn']['roofline']['frac'])"
