// stubs of the HIP translation units for a sanitizer build of the host code (CPU only, injected backend)
#include "spg_internal.h"
namespace spg {
int hip_backend_create(int, spg_backend *, char *, size_t) { return SPG_ENODEV; }
void hip_backend_destroy(spg_backend *) {}
void *hip_backend_stream(spg_backend *) { return nullptr; }
const char *hip_backend_error(spg_backend *) { return ""; }
int hip_backend_launches(spg_backend *) { return 0; }
int hip_backend_device(spg_backend *) { return -1; }
void hip_backend_profile(spg_backend *, int) {}
void hip_backend_profile_read(spg_backend *, double *, double *, long long *, long long *) {}
void hip_backend_profile_read_worker(spg_backend *, double *, double *, long long *, long long *) {}
void hip_backend_profile_read_big(spg_backend *, double *, double *, long long *, int *) {}
int hip_backend_end_of_call(spg_backend *) { return 0; }
int hip_stream_open(spg_backend *, int, int, int, StreamPort *) { return 1; }
void hip_stream_close(spg_backend *, const StreamPort *, double, long long) {}
int hip_la_test(int, int, int, int, int, int, double *, int, int, double *, int, int, double *, int, int, int *) { return SPG_ENODEV; }
int hip_big_glc_dense(void *, const DenseGraphIn &, int, int, int, int64_t, double *, int, int, double *, double *, char *, size_t) { return SPG_ENODEV; }
int hip_dense_information(void *, const DenseGraphIn &, int, double *, char *, size_t) { return SPG_ENODEV; }
int hip_dense_covariance(void *, const DenseGraphIn &, int, double *, char *, size_t) { return SPG_ENODEV; }
int rccl_get_unique_id(void *, char *, size_t) { return SPG_ENODEV; }
int rccl_comm_create(int, int, int, const void *, void **, char *, size_t) { return SPG_ENODEV; }
int rccl_allgather_f64(void *, void *, int64_t, int64_t, void *, char *, size_t) { return SPG_ENODEV; }
void rccl_comm_destroy(void *) {}
int hip_dense_kld(void *, const DenseGraphIn &, const DenseGraphIn &, int, int, const int64_t *, const int64_t *, spg_kld_terms &, char *, size_t) { return SPG_ENODEV; }
int hip_dense_optimize(void *, const DenseGraphIn &, int, int, spg_optimize_stats &, char *, size_t) { return SPG_ENODEV; }
int hip_sparse_optimize(void *, const DenseGraphIn &, int, int, spg_optimize_stats &, char *, size_t) { return SPG_ENODEV; }
int hip_sparse_kld(void *, const DenseGraphIn &, const DenseGraphIn &, const uint8_t *, const int32_t *, const int32_t *, int, const int64_t *, const int64_t *, spg_kld_terms &, char *, size_t) { return SPG_ENODEV; }
int hip_sparse_cov_blocks(void *, const DenseGraphIn &, int, const int32_t *, int, double *, spg_cov_stats &, char *, size_t) { return SPG_ENODEV; }
int hip_sparse_cov_solve(void *, const DenseGraphIn &, const int32_t *, const int32_t *, const int64_t *, int32_t, int64_t, int64_t, double *, spg_cov_solve_stats &, char *, size_t) { return SPG_ENODEV; }
int hip_sparse_relative(void *, const DenseGraphIn &, const int32_t *, const int32_t *, const int64_t *, int32_t, int64_t, int64_t, const int32_t *, const int32_t *, const int32_t *, int, const double *, double *, double *, double *, double *, double *, int32_t *, spg_cov_solve_stats &, char *, size_t) { return SPG_ENODEV; }
int hip_sparse_select(void *, const DenseGraphIn &, const int32_t *, const int32_t *, const int64_t *, int32_t, int64_t, int64_t, const int32_t *, const int32_t *, const int32_t *, const int32_t *, int, const double *, int, double, double, int32_t *, double *, double *, int32_t *, int *, spg_select_stats &, char *, size_t, const GreedyLazyIn *) { return SPG_ENODEV; }
int hip_sparse_prune(void *, const DenseGraphIn &, const int32_t *, const int32_t *, const int64_t *, int32_t, int64_t, int64_t, const int32_t *, const int32_t *, const int32_t *, int, int, double, double, double, int32_t *, double *, double *, double *, double *, int32_t *, int *, spg_prune_stats &, char *, size_t, const GreedyLazyIn *) { return SPG_ENODEV; }
int hip_sparse_detect(void *, const DenseGraphIn &, const int32_t *, const int32_t *, const int64_t *, int32_t, int64_t, int64_t, const int32_t *, const int32_t *, const int32_t *, int, int, double, double, int32_t *, double *, double *, double *, double *, int32_t *, int *, spg_outlier_stats &, char *, size_t, const GreedyLazyIn *) { return SPG_ENODEV; }
int hip_sparse_compat(void *, const DenseGraphIn &, const int32_t *, const int32_t *, const int64_t *, int32_t, int64_t, int64_t, const int32_t *, const int32_t *, const int32_t *, const int32_t *, int, const double *, int, double, double, const double *, const CompatOut &, int *, spg_compat_stats &, char *, size_t) { return SPG_ENODEV; }
int hip_max_clique(void *, int, const uint64_t *, int32_t *, int *, int32_t *, char *, size_t) { return SPG_ENODEV; }
int hip_propose_search(void *, const ProposeIn &, bool, std::vector<int32_t> &, std::vector<double> &, std::vector<double> &, spg_propose_stats &, char *, size_t) { return SPG_ENODEV; }
int hip_propose_gate(void *, const DenseGraphIn &, const int32_t *, const int32_t *, const int64_t *, int32_t, int64_t, int64_t, const int32_t *, const int32_t *, const int32_t *, int, double, double *, double *, spg_cov_solve_stats &, char *, size_t) { return SPG_ENODEV; }
int hip_select_removals(void *, const RemovalsIn &, bool, std::vector<int32_t> &, std::vector<int32_t> &, std::vector<double> &, spg_removal_stats &, char *, size_t) { return SPG_ENODEV; }
int hip_sparse_marginal_kld(void *, const DenseGraphIn &, const DenseGraphIn &, const int32_t *, const int32_t *, int, const int64_t *, const int64_t *, double *, spg_cov_stats &, char *, size_t) { return SPG_ENODEV; }
}
