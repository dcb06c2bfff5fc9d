OUT=${OUT:?set OUT to the output directory}
mkdir -p $OUT/r4final
timeout 1200 python bench.py --full 2>$OUT/r4final/bench.err | tail -1 > $OUT/r4final/bench_default.json
python tools/dbg/show_bench.py $OUT/r4final/bench_default.json
bash tools/prof_bench.sh r04final > $OUT/r4final/kernel_trace_summary.txt 2>&1
head -8 $OUT/r4final/kernel_trace_summary.txt | cut -c1-200
