"""AMP-Net inference at a chosen matrix precision: amp_test.test with `precision=` as its last keyword.

pointNet/amp_test.py builds its two networks without a precision, so they follow what the calling thread sees; this driver resolves the
precision (argument, then AMPNET_PRECISION, then the library default), logs it once and runs amp_test.test inside that
_lib.precision_scope -- every launch of the run, segment_file and segment_files included, is made on this thread."""
from .._lib import describe_precision, precision_scope, resolve_precision
from . import amp_test


def test(dataset_path, out_path, n_points, number_of_workers, model_checkpoint, path_list_files, cluster_dir='k_means_25',
         device='cuda', allow_pickle=None, files_per_launch=1, precision=None):
    """amp_test.test's arguments, files and return value; precision: 'fp32', 'f32x3', 'bf16', 'bf16_train', 'bf16_store', or None:
    AMPNET_PRECISION from the environment, else the library's process-wide default."""
    precision = resolve_precision(precision)
    print("matrix precision:", describe_precision(precision), flush=True)
    with precision_scope(precision):
        return amp_test.test(dataset_path, out_path, n_points, number_of_workers, model_checkpoint, path_list_files, cluster_dir=cluster_dir,
                             device=device, allow_pickle=allow_pickle, files_per_launch=files_per_launch)
