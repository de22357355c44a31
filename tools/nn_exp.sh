# timing experiments on iba_nn_kernel at the bench shape, same box: the regular library, builds with -DIBA_NN_EXP=1 (the nearest listed neighbour's 48 bytes not
# fetched) and =2 (the loads of the list pass alone, no picks), and the IBA_NN_DBG cuts (1: block start-up only). Results of the experiments are invalid; times only.
# build first: make -C spatial-temporal-lidar-camera-calibration_amd/csrc OUT=../libiba_exp1.so CXXFLAGS="... -DIBA_NN_EXP=1"
export IBA_DEBUG_ENV=1
cd $GRAFT_REPO_ROOT
P=$GRAFT_REPO_ROOT/spatial-temporal-lidar-camera-calibration_amd
run() {
  env "$@" python3 bench.py --full --steps 20 --warmup 3 --settle 300 --no-cpu-baseline --no-extras 2>/dev/null | python3 -c "
import sys, json
d = json.loads(sys.stdin.read().strip().split('\n')[-1]); k = d['roofline']['kernel_ms']
print('$*', 'ms/step %.4f' % d['ms_per_step'], {a: round(b, 4) for a, b in k.items()})"
}
run A=0
for e in $(ls $P | grep -o 'libiba_exp[0-9]*.so'); do run IBA_LIB=$P/$e; done
run IBA_NN_DBG=1
run IBA_NN_DBG=3
run A=0
