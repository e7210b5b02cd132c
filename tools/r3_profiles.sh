#!/bin/bash
# developer script (GPU box): everything the round's profiles/ directory records
export TMPDIR=/tmp
O=gpurun_out/r3prof
mkdir -p $O
B="timeout -k 10 200 python bench.py --full"
$B > $O/bench_headline.json 2> $O/err.log; echo "headline rc=$?"
$B --delta 1.4901161193847656e-08 --cpu-evals 0 > $O/bench_headline_delta_sqrteps.json 2>> $O/err.log; echo "delta rc=$?"
$B --workload "random-eqqp n=1e5 m=1e4 nnz=1e6" --cpu-evals 2 > $O/bench_cfg2.json 2>> $O/err.log; echo "cfg2 rc=$?"
$B --workload "aug2dc-like N=100" --delta 1.4901161193847656e-08 --cpu-evals 1 --steps 5 --repeats 3 > $O/bench_cfg4.json 2>> $O/err.log; echo "cfg4 rc=$?"
$B --workload "dense-block n=4096 m=2048" --steps 10 --warmup 2 > $O/bench_dense_block.json 2>> $O/err.log; echo "dense rc=$?"
$B --op hprod --cpu-evals 2 > $O/bench_hprod.json 2>> $O/err.log; echo "hprod rc=$?"
$B --op hprod --hessian-approx 1 --cpu-evals 0 > $O/bench_hprod_val1.json 2>> $O/err.log; echo "hprod val1 rc=$?"
$B --op hprod-solves --cpu-evals 0 > $O/bench_hprod_solves.json 2>> $O/err.log; echo "hprod-solves rc=$?"
$B --op extras --cpu-evals 0 > $O/bench_extras.json 2>> $O/err.log; echo "extras rc=$?"
$B --pointers host --cpu-evals 0 > $O/bench_host_pointers.json 2>> $O/err.log; echo "host rc=$?"
$B --pointers host+jac --cpu-evals 0 > $O/bench_host_pointers_jac.json 2>> $O/err.log; echo "host+jac rc=$?"
$B --force-shard --cpu-evals 0 > $O/bench_force_shard_world1.json 2>> $O/err.log; echo "force-shard rc=$?"
rm -rf $O/ks; timeout -k 10 150 rocprofv3 --kernel-trace --stats --output-format csv -d $O/ks -o k -- python3 bench.py --full --steps 20 --warmup 3 --cpu-evals 0 --repeats 2 > $O/ks.log 2>&1; echo "kernel stats rc=$?"
python3 tools/timeline.py $O/ks/k_kernel_trace.csv k_startup > $O/timeline.txt 2>&1
rm -rf $O/pf; timeout -k 10 150 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pf -o f -- python3 bench.py --steps 2 --warmup 1 --cpu-evals 0 --repeats 1 --no-roofline-pass > $O/pf.log 2>&1; echo "pmc fetch rc=$?"
rm -rf $O/pw; timeout -k 10 150 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pw -o w -- python3 bench.py --steps 2 --warmup 1 --cpu-evals 0 --repeats 1 --no-roofline-pass > $O/pw.log 2>&1; echo "pmc write rc=$?"
python3 tools/pmc_traffic.py $O/pf/f_counter_collection.csv $O/pw/w_counter_collection.csv 15 > $O/pmc_traffic.json 2> $O/pmc_traffic.err; echo "pmc post rc=$?"
rm -rf $O/dks; timeout -k 10 150 rocprofv3 --kernel-trace --stats --output-format csv -d $O/dks -o d -- python3 bench.py --workload "dense-block n=4096 m=2048" --steps 5 --warmup 1 --cpu-evals 0 --repeats 1 > $O/dks.log 2>&1; echo "dense stats rc=$?"
rm -f $O/ks/k_kernel_trace.csv $O/pf/f_kernel_trace.csv $O/pw/w_kernel_trace.csv $O/dks/d_kernel_trace.csv
ls $O
