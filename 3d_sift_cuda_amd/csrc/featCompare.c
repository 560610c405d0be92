/*
 * featCompare.c -- two intensity images on one grid scored against each other: the mutual information of their joint histogram and
 * its normalised form, the correlation coefficient and, on one intensity scale, the RMS difference (sift3d_image_similarity,
 * DESIGN.md section 7o).  The tool for asking how well a featResample warp matches the fixed image, across scanners and sequences
 * too, where a correlation coefficient says nothing.  Beyond the reference.
 *
 *   featCompare [-b<bins>] [-s] [-l <labels>] [-d<N>] <image a> <image b> [<out.txt>]
 *
 * Without <out.txt> the lines go to the standard output.  Every exit goes through one place that releases what was read.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_common.h"

static void print_options(void)
{
    printf("Similarity of two images on one grid v1.0\n");
    printf("Usage: %s [options] <image a> <image b> [<out.txt>]\n", "featCompare");
    printf("  <image a>, <image b>: nifti (.nii,.hdr,.nii.gz) on one grid; voxels that are not finite in either image are left out.\n");
    printf("  <out.txt>: the lines (default: the standard output): the ranges, the voxels counted and left out, then\n");
    printf("             \"mi nmi rho rms h_a h_b h_ab\": mutual information (nats), (h_a + h_b) / h_ab, correlation coefficient,\n");
    printf("             RMS difference (-s only, else nan), the entropies of a, of b and of the pair.\n");
    printf(" [options]\n");
    printf("  -b[8|16|32|64] : bins per image of the joint histogram (default: 64).\n");
    printf("  -s         : both images on one intensity scale: b is binned with a's range, and the RMS difference is given.\n");
    printf("  -l <labels>: a label image on the same grid (integers 0 .. 65535, NaN where unlabelled): also one line per label with the\n");
    printf("               voxels counted, the correlation coefficient and the RMS difference inside it (at most %d labels).\n", SIFT3D_SIMILARITY_MAX_LABELS);
    printf("  -d[0-9]    : set device id to be used.\n");
}

int main(int argc, char **argv)
{
    sift3d_similarity_params p;
    sift3d_similarity_defaults(&p);
    const char *l_path = NULL;
    int arg = 1;
    while (arg < argc && argv[arg][0] == '-' && argv[arg][1] != 0) {
        switch (argv[arg][1]) {
        case 'b':
            if (cli_int(argv[arg] + 2, 8, 64, &p.bins) != 0 || (p.bins != 8 && p.bins != 16 && p.bins != 32 && p.bins != 64))
                return cli_refuse(print_options, "bad number of bins: %s", argv[arg]);
            break;
        case 's':
            if (!cli_bare(argv[arg])) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            p.same_scale = 1;
            break;
        case 'l':
            if (!cli_bare(argv[arg]) || arg + 1 >= argc) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            l_path = argv[++arg];
            break;
        case 'd':
            if ((p.device = cli_device(argv[arg])) < 0) return cli_refuse(print_options, "unknown device: %s", argv[arg] + 2);
            break;
        default:
            return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
        }
        arg++;
    }
    if (argc - arg < 2 || argc - arg > 3) {
        print_options();
        return -1;
    }
    const char *a_path = argv[arg], *b_path = argv[arg + 1], *out_path = argc - arg == 3 ? argv[arg + 2] : NULL;
    nifti_min_image a, b, l;
    sift3d_similarity_record *rec = NULL;
    sift3d_similarity_label_record *lrec = NULL;
    char *text = NULL;
    FILE *o = NULL;
    int rc = -1;
    memset(&a, 0, sizeof a);
    memset(&b, 0, sizeof b);
    memset(&l, 0, sizeof l);
    if (cli_read_image(a_path, &a) != 0) goto done;
    if (cli_read_image(b_path, &b) != 0) goto done;
    if (l_path && cli_read_image(l_path, &l) != 0) goto done;
    if (a.nx != b.nx || a.ny != b.ny || a.nz != b.nz) {
        printf("Error: the images are not on one grid: %d x %d x %d voxels against %d x %d x %d\n", a.nx, a.ny, a.nz, b.nx, b.ny, b.nz);
        goto done;
    }
    if (l_path && (a.nx != l.nx || a.ny != l.ny || a.nz != l.nz)) {
        printf("Error: the labels are not on the images' grid: %d x %d x %d voxels against %d x %d x %d\n", a.nx, a.ny, a.nz, l.nx, l.ny, l.nz);
        goto done;
    }
    rec = (sift3d_similarity_record *)malloc(sizeof *rec);
    lrec = (sift3d_similarity_label_record *)malloc(sizeof *lrec * SIFT3D_SIMILARITY_MAX_LABELS);
    if (!rec || !lrec) {
        printf("Error: insufficient memory.\n");
        goto done;
    }
    char err[512] = "";
    int32_t n_labels = 0;
    if (sift3d_image_similarity(a.data, b.data, l_path ? l.data : NULL, a.nx, a.ny, a.nz, &p, rec, lrec, &n_labels, err, sizeof err) != SIFT3D_OK) {
        printf("Error: could not compare the images: %s\n", err);
        goto done;
    }
    const int64_t need = sift3d_similarity_report_text(rec, l_path ? lrec : NULL, n_labels, NULL, 0);
    text = need >= 0 ? (char *)malloc((size_t)need + 1) : NULL;
    if (!text || sift3d_similarity_report_text(rec, l_path ? lrec : NULL, n_labels, text, need + 1) != need) {
        printf("Error: insufficient memory.\n");
        goto done;
    }
    if (!(o = cli_open_out(out_path))) goto done;
    fprintf(o, "# featCompare v1.0 bins %d\n%s", (int)rec->bins, text);
    rc = cli_close_out(o, out_path);
    o = NULL;
done:
    if (o && out_path) fclose(o);
    free(text);
    free(lrec);
    free(rec);
    nifti_min_free(&a);
    nifti_min_free(&b);
    nifti_min_free(&l);
    return rc;
}
