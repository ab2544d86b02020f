"""tools/launch_diff.py on two small kernel-trace CSVs: the same launches in another order are equal, one changed grid is a difference."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("launch_diff", os.path.join(ROOT, "tools", "launch_diff.py"))
ld = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ld)

HEADER = "Kind,Kernel_Name,LDS_Block_Size,Workgroup_Size_X,Workgroup_Size_Y,Workgroup_Size_Z,Grid_Size_X,Grid_Size_Y,Grid_Size_Z"
ROWS = [
    'KERNEL_DISPATCH,"void k_mm_bwd<8, 16, false, true, false, true>(Src2<bf16>, float const*, int)",65536,512,1,1,262144,1,1',
    'KERNEL_DISPATCH,"k_bce_fwd(float const*, float*, long)",0,256,1,1,4096,2,1',
    'KERNEL_DISPATCH,"void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>>(int)",0,256,1,1,512,1,1',
]


def _trace(tmp_path, name, rows):
    d = tmp_path / name / "host" / "1234"  # rocprofv3 nests its output by host and process
    d.mkdir(parents=True)
    (d / "1234_kernel_trace.csv").write_text("\n".join([HEADER] + rows) + "\n")
    return str(tmp_path / name)


def test_equal_then_one_grid_changed(tmp_path, capsys):
    old = _trace(tmp_path, "old", ROWS)
    same = _trace(tmp_path, "same", ROWS[::-1])  # a multiset: the order of the launches does not count
    assert ld.main(["launch_diff", old, same]) == 0
    assert capsys.readouterr().out.strip() == "launch_diff: 2 / 2 launches of k_* kernels, 2 distinct (kernel, grid, block, LDS) keys, 0 differ"

    changed = _trace(tmp_path, "changed", [ROWS[0].replace(",262144,1,1", ",131072,1,1")] + ROWS[1:])
    assert ld.main(["launch_diff", old, changed]) == 1
    out = capsys.readouterr().out.strip().split("\n")
    assert out[:2] == [
        "DIFF  k_mm_bwd<8, 16, false, true, false, true>  grid=(131072, 1, 1) block=(512, 1, 1) lds=65536: 0 -> 1 launches",
        "DIFF  k_mm_bwd<8, 16, false, true, false, true>  grid=(262144, 1, 1) block=(512, 1, 1) lds=65536: 1 -> 0 launches",
    ]
    assert out[2].endswith("3 distinct (kernel, grid, block, LDS) keys, 2 differ")
