"""--vcf on the command line (no GPU needed): the option is listed, and an unwritable VCF path fails at once, before the GPU is touched."""
import os
import subprocess

from helpers import GOLDEN, ROOT

EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CWD = os.path.join(GOLDEN, "chr21")


def test_unwritable_vcf_path_fails_before_any_gpu_work():
    bad = "/nonexistent/dir/x.vcf"
    p = subprocess.run([EXE, "--vcf", bad, "inv_del_bam_config"], cwd=CWD, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, BDX_FOREGROUND="1"), timeout=60)
    err = p.stderr.decode()
    assert p.returncode == 1, err
    # (the file is opened right after the configuration: no GPU context, no decode -- on a machine without a GPU the message is
    # still this one, not bdx_create's)
    assert "ERROR:" in err and bad in err and "VCF" in err, err
    assert "bdx_create" not in err and p.stdout == b""


def test_usage_lists_the_vcf_option():
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1
    assert "--vcf FILE" in p.stderr.decode()
