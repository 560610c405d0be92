"""CPU suite: the command lines beyond the reference refuse a bad command line before they open a file or ask for a device (DESIGN.md
section 7p) -- per tool a table of command lines with the error line each prints, spelled here, above the tool's own usage text; and
cli_common.c under the sanitizers as a stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

R4 = ["f.nii", "m.nii", "m.trans.txt", "o.nii"]
C4 = ["a.nii", "1.trans.txt", "2.trans.txt", "o"]
F6 = ["t.nii", "o.nii", "a", "b", "c", "-"]
L2 = ["a.nii", "b.nii"]
UNKNOWN = "unknown command line argument: "
FOUR = "every atlas takes four arguments: <atlas image> <atlas labels> <atlas.trans.txt> <atlas.field.nii|->"

# (argv, the text after "Error: " or None for the usage alone).  No case reaches a file: none exists.  No case asks for the number of
# devices: -d, -dx and -d0x are refused before that.
CASES = {
    "FEATRESAMPLE": [
        ([], None), (["f.nii"], None), (R4 + ["more"], None), (["-w", "-n", "-f1", "-i", "-i0", "-i8", "-c", "-r", "-j"] + R4[:3], None),
        (["-wx", "-Wx", "-ws", "-nx"] + R4[:3], None),                                  # -w and -n take trailing characters
        (["-"] + R4, UNKNOWN + "-"), (["-x"] + R4, UNKNOWN + "-x"), (["-lx"] + R4, UNKNOWN + "-lx"), (["-i", "-cx"] + R4, UNKNOWN + "-cx"),
        (["-rx"] + R4, UNKNOWN + "-rx"), (["-jx"] + R4, UNKNOWN + "-jx"), (["-f"] + R4, "bad fill value: -f"), (["-f1x"] + R4, "bad fill value: -f1x"),
        (["-d"] + R4, "unknown device: "), (["-dx"] + R4, "unknown device: x"), (["-d0x"] + R4, "unknown device: 0x"),
        (["-i3x"] + R4, "bad number of rounds: -i3x"), (["-i-1"] + R4, "bad number of rounds: -i-1"), (["-i9"] + R4, "bad number of rounds: -i9"),
        (["-i99999999999999999999"] + R4, "bad number of rounds: -i99999999999999999999"), (["-u"], "-u needs a field file"),
        (["-ux", "f.field.nii"] + R4, "-u needs a field file"), (["-l", "-n"] + R4, "-n and -l are two interpolations: give one"),
        (["-nx", "-l", "-c"] + R4, "-n and -l are two interpolations: give one"), (["-c"] + R4, "-c needs -i"),
        (["-c", "-l", "-n"] + R4[:3], None),                                            # the count of the arguments comes first
    ],
    "FEATCOMPOSE": [
        ([], None), (["a.nii"], None), (C4 + ["more"], None), (["-w", "-wsx", "-h2.5", "-u1", "1.field.nii", "-u2", "2.field.nii"] + C4[:3], None),
        (["-"] + C4, UNKNOWN + "-"), (["-x"] + C4, UNKNOWN + "-x"), (["-d"] + C4, "unknown device: "), (["-dx"] + C4, "unknown device: x"),
        (["-d0x"] + C4, "unknown device: 0x"), (["-h"] + C4, "bad spacing: -h"), (["-h0"] + C4, "bad spacing: -h0"), (["-h-1"] + C4, "bad spacing: -h-1"),
        (["-h2x"] + C4, "bad spacing: -h2x"), (["-hnan"] + C4, "bad spacing: -hnan"), (["-u", "1.field.nii"] + C4, "-u1 and -u2 need a field file"),
        (["-u3", "1.field.nii"] + C4, "-u1 and -u2 need a field file"), (["-u1x", "1.field.nii"] + C4, "-u1 and -u2 need a field file"),
        (["-u2"], "-u1 and -u2 need a field file"),
    ],
    "FEATFUSE": [
        ([], None), (["-"], None), (["-", "-x"], None), (["t.nii", "o.nii"], None), (["-w", "-c", "-b1", "-b6", "-p0", "-p2", "-l", "-fnan", "-t", "truth.nii", "-m", "t.nii"], None),
        (["-b2", "-s1", "-s3", "t.nii", "o.nii"], None), (F6[:5], FOUR), (F6 + ["a"], FOUR), (["-", "-x"] + F6, FOUR),
        (F6[:2] + F6[2:] * 33, "more than 32 atlases"), (["-x"] + F6, UNKNOWN + "-x"), (["-cx"] + F6, UNKNOWN + "-cx"), (["-lx"] + F6, UNKNOWN + "-lx"),
        (["-mx"] + F6, UNKNOWN + "-mx"), (["-b"] + F6, "bad patch half-width: -b"), (["-b0"] + F6, "bad patch half-width: -b0"), (["-b7"] + F6, "bad patch half-width: -b7"),
        (["-b2x"] + F6, "bad patch half-width: -b2x"), (["-p-1"] + F6, "bad power: -p-1"), (["-p3"] + F6, "bad power: -p3"), (["-s"] + F6, "bad search radius: -s"),
        (["-s0"] + F6, "bad search radius: -s0"), (["-s4"] + F6, "bad search radius: -s4"), (["-s1x"] + F6, "bad search radius: -s1x"),
        (["-f"] + F6, "bad fill value: -f"), (["-f1x"] + F6, "bad fill value: -f1x"), (["-t"], "-t needs a label image: -t"),
        (["-tx", "truth.nii"] + F6, "-t needs a label image: -tx"), (["-d"] + F6, "unknown device: "), (["-dx"] + F6, "unknown device: x"), (["-d0x"] + F6, "unknown device: 0x"),
        (["-p0", "-s1"] + F6, "a search needs weights to search by: -s with -p0"), (["-s1", "-p0"] + F6, "a search needs weights to search by: -s with -p0"),
        (["-b4", "-s3"] + F6, "the patch half-width plus the search radius must not exceed 6: -b with -s"),
        (["-b5", "-s2", "-p0", "-m"], "a search needs weights to search by: -s with -p0"),      # the order of the checks after the loop
        (["-b5", "-s2", "-m"], "the patch half-width plus the search radius must not exceed 6: -b with -s"),
        (["-m", "t.nii"], "the surface distances are taken to a truth: -m without -t"),
    ],
    "FEATOVERLAP": [
        ([], None), (["-"], None), (["-", "-x"] + L2, None), (["a.nii"], None), (L2 + ["o.txt", "more"], None), (["-m", "-z", "a.nii"], None),
        (["-x"] + L2, UNKNOWN + "-x"), (["-mx"] + L2, UNKNOWN + "-mx"), (["-zx"] + L2, UNKNOWN + "-zx"), (["-d"] + L2, "unknown device: "),
        (["-dx"] + L2, "unknown device: x"), (["-d0x"] + L2, "unknown device: 0x"),
    ],
    "FEATCLEAN": [
        ([], None), (["-"], None), (["-", "-x", "a.nii"], None), (["a.nii"], None), (L2 + ["more"], None),
        (["-v1", "-v16777216", "-c6", "-c26", "-r1", "-r16", "-t", "truth.nii", "-m", "a.nii"], None), (["-x"] + L2, UNKNOWN + "-x"), (["-mx"] + L2, UNKNOWN + "-mx"),
        (["-v"] + L2, "bad minimum of voxels: -v"), (["-v0"] + L2, "bad minimum of voxels: -v0"), (["-v16777217"] + L2, "bad minimum of voxels: -v16777217"),
        (["-v8x"] + L2, "bad minimum of voxels: -v8x"), (["-c"] + L2, "bad connectivity: -c"), (["-c18"] + L2, "bad connectivity: -c18"), (["-c6x"] + L2, "bad connectivity: -c6x"),
        (["-c06"] + L2, "bad connectivity: -c06"), (["-r"] + L2, "bad number of rounds: -r"), (["-r0"] + L2, "bad number of rounds: -r0"), (["-r17"] + L2, "bad number of rounds: -r17"),
        (["-r2x"] + L2, "bad number of rounds: -r2x"), (["-t"], "-t needs a label image: -t"), (["-tx", "truth.nii"] + L2, "-t needs a label image: -tx"),
        (["-d"] + L2, "unknown device: "), (["-dx"] + L2, "unknown device: x"), (["-d0x"] + L2, "unknown device: 0x"),
        (["-m"] + L2, "the surface distances are taken to a truth: -m without -t"), (["-m", "a.nii"], "the surface distances are taken to a truth: -m without -t"),
    ],
    "FEATCOMPARE": [
        ([], None), (["-"], None), (["-", "-x"] + L2, None), (["a.nii"], None), (L2 + ["o.txt", "more"], None), (["-b8", "-b16", "-b32", "-b64", "-s", "-l", "l.nii", "a.nii"], None),
        (["-x"] + L2, UNKNOWN + "-x"), (["-sx"] + L2, UNKNOWN + "-sx"), (["-l"], UNKNOWN + "-l"), (["-lx", "l.nii"] + L2, UNKNOWN + "-lx"),
        (["-b"] + L2, "bad number of bins: -b"), (["-b7"] + L2, "bad number of bins: -b7"), (["-b9"] + L2, "bad number of bins: -b9"), (["-b12"] + L2, "bad number of bins: -b12"),
        (["-b65"] + L2, "bad number of bins: -b65"), (["-b128"] + L2, "bad number of bins: -b128"), (["-b8x"] + L2, "bad number of bins: -b8x"),
        (["-d"] + L2, "unknown device: "), (["-dx"] + L2, "unknown device: x"), (["-d0x"] + L2, "unknown device: 0x"),
    ],
}


@pytest.mark.parametrize("tool", sorted(CASES))
def test_refusals_print_the_error_line_and_the_usage(built, tool, tmp_path):
    exe = getattr(built, tool)
    run = lambda argv: subprocess.run([exe] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    usage = run([]).stdout
    assert usage.count("\n") > 5 and "Usage: feat%s%s " % (tool[4], tool[5:].lower()) in usage and "Error" not in usage
    assert len(CASES[tool]) >= 6 and any("-" in argv for argv, _ in CASES[tool])
    for argv, error in CASES[tool]:
        r = run(argv)
        assert r.returncode == 255 and r.stderr == "", (argv, r.returncode, r.stderr[-500:])
        assert r.stdout == ("Error: %s\n" % error if error is not None else "") + usage, (argv, r.stdout[:300])
    assert os.listdir(str(tmp_path)) == []


def test_cli_common_under_sanitizers(built, tmp_path):
    """cli_common.c, field_io.c, nifti_min.c and tests/cli_common_san.c as one program, with and without -fsanitize=address,undefined:
    both exit clean and print the same lines, and those say what the option loops rely on"""
    csrc = os.path.join(ROOT, "3d_sift_cuda_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "cli_common_san.c")] + [os.path.join(csrc, f) for f in ("cli_common.c", "field_io.c", "nifti_min.c")]
    base = ["cc", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    out = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])):
        exe, work = str(tmp_path / ("cli_common_" + name)), tmp_path / ("work_" + name)
        work.mkdir()
        subprocess.run(base + flags + ["-o", exe] + src + ["-lz", "-lm"], check=True)
        r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        out[name] = r.stdout
    text = out["san"]
    assert text == out["plain"]
    assert text.startswith("Error: -c needs -i\nusage\nrefuse -1\nError: bad power: -p3\nusage\nrefuse -1\nError: unknown device: \nusage\nrefuse -1\nbare 1 0\n")
    for s in ("", " ", "+", "-", "x", "3x", "x3", "3 ", "0x3", "3.0", "99999999999999999999", "-99999999999999999999"):
        assert "int [%s] -5..5: -1 -777\n" % s in text, s
    for s, v in ((" 3", 3), ("+3", 3), ("-3", -3), ("03", 3)):
        assert "int [%s] -5..5: 0 %d\n" % (s, v) in text, s
    for lo, hi in ((0, 8), (1, 16), (1, 6), (0, 2), (1, 3), (1, 16777216), (8, 64)):      # every range an option has, at and around its bounds
        for v in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1):
            assert "int [%d] %d..%d: %s\n" % (v, lo, hi, "0 %d" % v if lo <= v <= hi else "-1 -777") in text, (v, lo, hi)
    big = 2 ** 31
    assert "int [%d] 0..%d: -1 -777\nint [%d] 0..%d: 0 %d\nint [%d] %d..0: 0 %d\nint [%d] %d..0: -1 -777\n" % (big, big - 1, big - 1, big - 1, big - 1, -big, -big, -big,
                                                                                                    -big - 1, -big) in text
    for s in ("", " ", "+", "-", "x", "1x", "1 ", "1e"):
        assert "float [%s]: -1\n" % s in text, s
    for s, v in ((" 1", "1"), ("+1.5", "1.5"), ("-1.5", "-1.5"), ("1e3", "1000"), ("nan", "nan"), ("inf", "inf"), ("-inf", "-inf"), ("1e999", "inf"), (".5", "0.5")):
        assert "float [%s]: 0 %s\n" % (s, v) in text, s
    assert "world 1 2 2 1 1\n" in text
    for s, v in (("-d", -1), ("-dx", -1), ("-d0", 0), ("-d1", 1), ("-d2", -1), ("-d9", -1), ("-d0x", -1), ("-d10", -1), ("-d/", -1), ("-d:", -1)):
        assert "device [%s] %d\n" % (s, v) in text, s                               # the program states two devices
    assert text.count("path ") == 9 and all(line.endswith(" 1") for line in text.split("\n") if line.startswith("path "))
    assert "path 0+0: 0  1\n" in text and "path 7+10: 17 out.nii.clean.txt 1\n" in text and "path 10000+10: 10010 (long) 1\n" in text
    q, s = " ".join(str(k) for k in range(1, 13)) + " 0 0 0 1\n", " ".join(str(k) for k in range(101, 113)) + " 0 0 0 1\n"
    fallback = "Error: sform_code <= 0, using qto_xyz instead of sto_xyz\n"
    assert "sform_code 0 mode 1\nworld_matrix " + q + "vox2key is the matrix: 1\n" in text
    assert "sform_code 0 mode 2\n" + fallback + "world_matrix " + q + fallback + "vox2key is the matrix: 1\n" in text
    assert "sform_code 2 mode 1\nworld_matrix " + q + "vox2key is the matrix: 1\n" in text
    assert "sform_code 2 mode 2\nworld_matrix " + s + "vox2key is the matrix: 1\n" in text and text.count(fallback) == 2
    assert "alloc capacity 72\nheader 1\nno field without a directory: 1\nread 0\nread back 4 3 2 2.5 -1 0.5 7.25 capacity 72 same 1\n" in text
    assert "Error: could not read displacement field file: cut.field.nii\nread cut -1\n" in text
    assert "Error: could not read displacement field file: none.field.nii\nread none -1\n" in text
    assert "Error: could not read input file: none.nii\nimage none -1\nstdout is stdout 1, closes 0\n" in text
    assert text.endswith("Error: could not write output file: nodir/o.txt\nopen none 1\nfile closes 0\n")
    assert open(str(tmp_path / "work_san" / "w.field.txt")).read() == "# nodes 4 3 2 spacing 2.500000 origin -1.000000 0.500000 7.250000 tail 7\n"
