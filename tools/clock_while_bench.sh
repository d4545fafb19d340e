# samples rocm-smi's clocks and power while bench.py's timed steps run (is the matrix pipe's ceiling a clock/power ceiling?)
#   bash tools/clock_while_bench.sh [OUTDIR]      (default bench_out/; --full: the second, unprofiled pass of the steps too)
OUT=${1:-bench_out}
mkdir -p $OUT
python3 bench.py --full --no-extras --no-cpu-baseline --no-emulation --steps 40 --warmup 3 > $OUT/bench_clk.json 2> $OUT/bench_clk.err &
BP=$!
sleep 8
for i in $(seq 1 40); do rocm-smi --showclocks --showpower 2>/dev/null | grep -i "sclk\|power\|mclk" | tr '\n' ' '; echo; sleep 0.2; done > $OUT/clk_samples.txt
wait $BP
tail -25 $OUT/clk_samples.txt
