"""Which kernel a launcher runs, held on the CPU: tests/host/launch_record.hip links the library's launcher objects against recording
stand-ins for the HIP runtime and prints one line per call of its sweep (gemm3 / fp32-A GEMM entries over shapes, operand formats,
ring depths, explicit tiles and every tuning switch; the persistent codec kernels over grid caps and masks).  The lines must equal
tests/golden/launch_table.txt.gz, recorded at the last commit that passed the tuning through globals: LaunchTuning as an argument
selects exactly the kernels, grids, LDS sizes and tile orders the globals selected."""
import gzip
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smalltts_amd", "csrc")


def test_every_launcher_picks_the_recorded_kernel_grid_and_lds():
    jobs = str(min(8, os.cpu_count() or 1))
    subprocess.run(["make", "-C", CSRC, "-j", jobs, "launch_record"], check=True, stdout=subprocess.DEVNULL)
    got = subprocess.run([os.path.join(CSRC, "build", "launch_record")], check=True, capture_output=True, text=True).stdout.splitlines()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "launch_table.txt.gz"), "rt") as f:
        head, *want = f.read().splitlines()
    assert head.startswith("# recorded at ")
    assert len(want) > 40000
    # the prototype's three lines (600 x 960 x 960, fp16, gated residual at ring depths 0 / 1 / 2) are in the table as measured then
    for deep, stages, lds in ((0, 2, 33024), (1, 4, 65792), (2, 8, 131328)):
        line = next(w for w in want if w.startswith(f"gemm3_resid1 f2 600x960x960 cfg-1 d{deep} "))
        assert line.endswith(f"-> gemm3_kernel<64,64,2,2,2,{stages},EpiResid<1>> grid=150,1,1 wg=256 lds={lds} nfast=0 stage16=1"), line
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diff, f"{len(diff)} lines differ, first: {diff[0]}"
    assert len(got) == len(want)
