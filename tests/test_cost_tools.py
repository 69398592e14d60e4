"""tools/costlib.py, what the tools/*_cost.py scripts share, as far as it runs without a GPU: the kernel-name normaliser and
the rocprofv3 CSV readers on a committed rocprofv3 file, the figures of summary(), and the rule that every cost tool parses
its arguments before torch, the package or the library are touched."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
STATS_CSV = os.path.join(ROOT, "profiles", "history", "r01_bench_configC_exact_kernel_stats.csv")
COST_TOOLS = ("adam", "antialias", "backward", "band_backward", "batch", "contrib", "densify", "init", "loss", "mcmc", "outputs",
              "sh_degree", "trainer_step")


@pytest.fixture(scope="module")
def costlib():
    sys.path.insert(0, TOOLS)
    try:
        import costlib
    finally:
        sys.path.remove(TOOLS)
    return costlib


def test_import_is_light():
    code = ("import sys; import costlib; "
            "sys.exit(1 if {'torch', 'vk3dgaussiansplatting_amd'} & set(sys.modules) else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=TOOLS).returncode == 0


@pytest.mark.parametrize("raw, name", [
    ("void gs::k_splat_offsets<gs::BwdSource<true> >(gs::BwdSource<true>, unsigned int*)", "k_splat_offsets<gs::BwdSource<true>>"),
    ("gs::k_count(gs::SortParams const*, unsigned int const*, unsigned int*, unsigned int*, unsigned int)", "k_count"),
    ("void gs::k_render<true>(gs::FrameParams, gs::SplatRaster const*, unsigned int const*, unsigned int const*, unsigned int*)",
     "k_render<true>"),
    ("__amd_rocclr_copyBuffer", "__amd_rocclr_copyBuffer"),
    # a template argument from an unnamed namespace carries a "(" of its own: the cut is behind the template arguments
    ("void gs::k_splat_offsets<gs::(anonymous namespace)::PruneSource>(gs::(anonymous namespace)::PruneSource, unsigned int*)",
     "k_splat_offsets<gs::(anonymousnamespace)::PruneSource>"),
])
def test_kernel_name(costlib, raw, name):
    assert costlib.kernel_name(raw) == name


def test_kernel_name_on_the_committed_file(costlib):
    with open(STATS_CSV) as f:
        text = f.read()
    for raw, name in (("gs::k_count(gs::SortParams const*,", "k_count"), ("void gs::k_render<true>(gs::FrameParams,", "k_render<true>")):
        line = next(ln for ln in text.splitlines() if ln.startswith('"' + raw))
        assert costlib.kernel_name(line.split('"')[1]) == name


def test_read_kernel_stats(costlib, tmp_path):
    nested = tmp_path / "host" / "1234"                          # the tools look for the file at any depth
    nested.mkdir(parents=True)
    shutil.copy(STATS_CSV, nested / "p_kernel_stats.csv")
    stats = costlib.read_kernel_stats(str(tmp_path))
    assert stats["k_scatter"].calls == 840
    assert stats["k_scatter"].average_us == pytest.approx(81.47994, abs=1e-5)
    assert {"k_count", "k_render<true>", "k_project", "__amd_rocclr_copyBuffer"} <= set(stats)
    assert costlib.kernel_us(stats, "k_scatter", "test") == pytest.approx(81.47994, abs=1e-5)
    assert costlib.kernel_us(stats, ("k_render<", "true"), "test") == pytest.approx(451.383785714, abs=1e-6)
    for missing in ("k_not_there", ("k_scatter", "<true>")):
        with pytest.raises(SystemExit) as e:
            costlib.kernel_us(stats, missing, "some_cost")
        assert "some_cost" in str(e.value) and "k_scatter" in str(e.value)


def test_read_kernel_trace(costlib, tmp_path):
    rows = [("void gs::k_bwd_rowsum_chain<true>(gs::FrameParams, float*)", 5000, 9000),
            ("gs::k_bwd_blend(gs::FrameParams)", 3000, 4500),
            ("void gs::k_splat_offsets<gs::BwdSource<true> >(gs::BwdSource<true>, unsigned int*)", 2000, 2250),
            ("void gs::k_splat_block_sums<gs::BwdSource<true> >(gs::BwdSource<true>, unsigned int*)", 100, 1100),
            ("__amd_rocclr_fillBufferAligned", 10, 20),
            ("void gs::k_splat_scan_blocks<gs::BwdSource<true> >(unsigned int*)", 1200, 1300)]
    (tmp_path / "out").mkdir()
    with open(tmp_path / "out" / "p_kernel_trace.csv", "w") as f:
        f.write('"Kind","Kernel_Name","Start_Timestamp","End_Timestamp"\n')
        for name, start, end in rows:
            f.write(f'"KERNEL_DISPATCH","{name}",{start},{end}\n')
    assert costlib.read_kernel_trace(str(tmp_path)) == [
        ("__amd_rocclr_fillBufferAligned", 1e-5), ("k_splat_block_sums<gs::BwdSource<true>>", 1e-3),
        ("k_splat_scan_blocks<gs::BwdSource<true>>", 1e-4), ("k_splat_offsets<gs::BwdSource<true>>", 2.5e-4),
        ("k_bwd_blend", 1.5e-3), ("k_bwd_rowsum_chain<true>", 4e-3)]


def test_no_csv_is_an_error(costlib, tmp_path):
    with pytest.raises(SystemExit):
        costlib.read_kernel_stats(str(tmp_path))
    with pytest.raises(SystemExit):
        costlib.read_kernel_trace(str(tmp_path))


def test_summary(costlib):
    assert costlib.summary([1.00004, 2.0, 4.0]) == (2.3333, 2.0, [1.0, 4.0])


def test_write_lines(costlib, tmp_path):
    path = tmp_path / "new" / "x_cost.txt"
    costlib.write_lines(str(path), "# header\n", [{"a": 1}, "# a remark", {"b": [1, 2]}])
    assert path.read_text() == '# header\n{"a": 1}\n# a remark\n{"b": [1, 2]}\n'


@pytest.mark.parametrize("tool", COST_TOOLS)
def test_help_needs_no_gpu(tool):
    """Arguments are parsed before torch and the library are touched: --help works where neither can be loaded."""
    blocked = "import sys; sys.modules['torch'] = None; sys.modules['vk3dgaussiansplatting_amd'] = None; import runpy; " \
              "sys.argv = sys.argv[1:]; sys.path.insert(0, sys.argv[0].rsplit('/', 1)[0]); runpy.run_path(sys.argv[0], run_name='__main__')"
    rc = subprocess.run([sys.executable, "-c", blocked, os.path.join(TOOLS, tool + "_cost.py"), "--help"], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    assert "usage:" in rc.stdout
