// Python bindings for the gfx950 kernel library (_hip_ops).
#include <torch/extension.h>

#include <vector>

// elementwise.hip
std::vector<at::Tensor> layernorm_fwd(const at::Tensor&, const at::Tensor&,
                                      const at::Tensor&, double);
std::vector<at::Tensor> add_layernorm_fwd(const at::Tensor&, const at::Tensor&,
                                          const at::Tensor&, const at::Tensor&,
                                          double);
std::vector<at::Tensor> layernorm_bwd(const at::Tensor&, const at::Tensor&,
                                      const at::Tensor&, const at::Tensor&,
                                      const at::Tensor&);
at::Tensor bias_gelu_fwd(const at::Tensor&, const at::Tensor&);
std::vector<at::Tensor> bias_gelu_bwd(const at::Tensor&, const at::Tensor&,
                                      const at::Tensor&);
std::vector<at::Tensor> masked_ce_fwd(const at::Tensor&, const at::Tensor&,
                                      const at::Tensor&);
at::Tensor masked_ce_bwd(const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, const at::Tensor&,
                         const at::Tensor&);
at::Tensor colsum(const at::Tensor&);
std::vector<at::Tensor> dropout_add_ln_fwd(const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&, double, double,
                                           const at::Tensor&);
at::Tensor mask_scale(const at::Tensor&, const at::Tensor&, double);
std::vector<at::Tensor> dropout_add_ln_bwd(const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&, double, bool);
void bump_counter(const at::Tensor&);
at::Tensor wgrad(const at::Tensor&, const at::Tensor&, long);
at::Tensor wgrad2(const at::Tensor&, const at::Tensor&, long);
at::Tensor gemm_nt(const at::Tensor&, const at::Tensor&,
                   c10::optional<at::Tensor>, bool);
at::Tensor gemm_tn(const at::Tensor&, const at::Tensor&, long, bool);
at::Tensor gemm_nn(const at::Tensor&, const at::Tensor&, bool);
std::vector<at::Tensor> gemm_nt_bias_gelu(const at::Tensor&,
                                          const at::Tensor&,
                                          const at::Tensor&, bool);
std::vector<at::Tensor> gemm_nn_dgelu(const at::Tensor&, const at::Tensor&,
                                      const at::Tensor&, const at::Tensor&);
at::Tensor embed3_fwd(const at::Tensor&, const at::Tensor&,
                      const at::Tensor&, const at::Tensor&,
                      const at::Tensor&);
std::vector<at::Tensor> embed3_bwd(const at::Tensor&, const at::Tensor&,
                                   const at::Tensor&, long, long, long);
std::vector<long> embed3_bwd_limits();
// crf.hip
std::vector<at::Tensor> crf_fwd(const at::Tensor&, const at::Tensor&,
                                const at::Tensor&, const at::Tensor&);
at::Tensor crf_viterbi(const at::Tensor&, const at::Tensor&,
                       const at::Tensor&);
// crf_pair.hip (T <= 64, both scan tables of a row in LDS): the loss kernel
// crf_fwd routes to; seqs_per_block 0 = the route's choice, 1 / 2 force it
std::vector<at::Tensor> crf_pair_fwd(const at::Tensor&, const at::Tensor&,
                                     const at::Tensor&, const at::Tensor&,
                                     int64_t);
// {pair kernel (1) or crf_wide.hip (0), waves per block, LDS bytes}
std::vector<int64_t> crf_fwd_route(int64_t, int64_t);
// {demis * dll[b], sum_b dtrans[b] * dll[b]} in one launch, new tensors
std::vector<at::Tensor> crf_grad_scale(const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&);
// crf_wide.hip (T <= 64, L <= 512): reached through crf_fwd / crf_viterbi,
// which route to it every shape their other kernels cannot launch
std::vector<at::Tensor> crf_wide_fwd(const at::Tensor&, const at::Tensor&,
                                     const at::Tensor&, const at::Tensor&);
at::Tensor crf_wide_viterbi(const at::Tensor&, const at::Tensor&,
                            const at::Tensor&);
// crf_posterior.hip (T <= 64, L <= 512): log-posterior of a given tag path,
// as two fp64 [B,L] arrays {span_a, span_b}
std::vector<at::Tensor> crf_path_posterior(const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&);
// crf_nbest.hip (T <= 64, L <= 512, k <= 8): the k best tag paths per row,
// {paths i32 [B,k,L], scores f32 [B,k]}; absent ranks: -inf, zero path
std::vector<at::Tensor> crf_nbest(const at::Tensor&, const at::Tensor&,
                                  const at::Tensor&, int64_t);
// {global backpointer route (0/1), waves per block, LDS bytes} of that launch
std::vector<int64_t> crf_nbest_route(int64_t, int64_t, int64_t);
// crf_partial.hip (T <= 64, L <= 512): partial-annotation CRF. allowed is one
// int64 word of permitted tags per position; {ll, demis, dtrans} of
// ll = log Z_allowed - log Z
std::vector<at::Tensor> crf_partial_fwd(const at::Tensor&, const at::Tensor&,
                                        const at::Tensor&, const at::Tensor&);
// {pair route (1) or split (0), waves per block, LDS bytes} of that launch
std::vector<int64_t> crf_partial_route(int64_t, int64_t);
// crf_constrained.hip (T <= 64, L <= 512): Viterbi under per-position
// allowed-tag words and per-tag allowed-transition words; {pred i32 [B,L],
// score f32 [B]}, rows without a path: -inf and a zero row
std::vector<at::Tensor> crf_viterbi_constrained(const at::Tensor&,
                                                const at::Tensor&,
                                                const at::Tensor&,
                                                const at::Tensor&,
                                                const at::Tensor&);
// softlexicon.hip
at::Tensor softlexicon_fwd(const at::Tensor&, const at::Tensor&,
                           const at::Tensor&);
std::vector<at::Tensor> softlexicon_bwd(const at::Tensor&, const at::Tensor&,
                                        const at::Tensor&, const at::Tensor&);
// adam.hip
void multi_tensor_adamw(std::vector<at::Tensor>, std::vector<at::Tensor>,
                        std::vector<at::Tensor>, std::vector<at::Tensor>,
                        std::vector<at::Tensor>, std::vector<double>,
                        std::vector<double>, double, double, double,
                        c10::optional<at::Tensor>);
at::Tensor multi_tensor_sumsq(std::vector<at::Tensor>);
void multi_tensor_scale(std::vector<at::Tensor>, const at::Tensor&);
std::vector<at::Tensor> adamw_build_meta(
    std::vector<at::Tensor>, std::vector<at::Tensor>, std::vector<at::Tensor>,
    std::vector<at::Tensor>, std::vector<at::Tensor>, std::vector<double>,
    std::vector<double>);
void multi_tensor_adamw_run(const at::Tensor&, long, long, bool, double,
                            double, double, c10::optional<at::Tensor>);
std::vector<at::Tensor> norm_build_meta(std::vector<at::Tensor>);
at::Tensor multi_tensor_sumsq_run(const at::Tensor&, long, const at::Tensor&);
void multi_tensor_scale_run(const at::Tensor&, long, const at::Tensor&);
void multi_tensor_adamw_tab_run(const at::Tensor&, long, long, bool,
                                std::vector<at::Tensor>,
                                std::vector<c10::optional<at::Tensor>>, double,
                                double, double, c10::optional<at::Tensor>,
                                c10::optional<at::Tensor>);
long grad_table_slots();
long sumsq_chunk_elems();
at::Tensor sumsq_build_chunks(std::vector<long>, std::vector<long>,
                              const at::Tensor&);
at::Tensor multi_tensor_sumsq_coef_run(const at::Tensor&, std::vector<long>,
                                       std::vector<long>,
                                       std::vector<c10::optional<at::Tensor>>,
                                       double);
// attention.hip
std::vector<at::Tensor> attn_fwd(const at::Tensor&, const at::Tensor&,
                                 const at::Tensor&, const at::Tensor&, double,
                                 double, c10::optional<at::Tensor>);
std::vector<at::Tensor> attn_bwd(const at::Tensor&, const at::Tensor&,
                                 const at::Tensor&, const at::Tensor&,
                                 const at::Tensor&, const at::Tensor&,
                                 const at::Tensor&, double, double,
                                 c10::optional<at::Tensor>);
std::vector<at::Tensor> attn_fwd_qkv(const at::Tensor&, const at::Tensor&,
                                     double, double,
                                     c10::optional<at::Tensor>);
std::vector<at::Tensor> attn_bwd_qkv(const at::Tensor&, const at::Tensor&,
                                     const at::Tensor&, const at::Tensor&,
                                     const at::Tensor&, double, double,
                                     c10::optional<at::Tensor>);
std::vector<at::Tensor> attn_bwd_qkv_dbias(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, double, double,
    c10::optional<at::Tensor>, const at::Tensor&);
// attention_tiled.hip
std::vector<at::Tensor> attn_tiled_fwd(const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, const at::Tensor&,
                                       double, double,
                                       c10::optional<at::Tensor>);
std::vector<at::Tensor> attn_tiled_bwd(const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, double, double,
                                       c10::optional<at::Tensor>);
std::vector<at::Tensor> attn_tiled_fwd_qkv(const at::Tensor&,
                                           const at::Tensor&, double, double,
                                           c10::optional<at::Tensor>);
std::vector<at::Tensor> attn_tiled_bwd_qkv(const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&,
                                           const at::Tensor&, double, double,
                                           c10::optional<at::Tensor>);
// tener.hip
std::vector<at::Tensor> tener_attn_fwd(const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, const at::Tensor&);
std::vector<at::Tensor> tener_attn_bwd(const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&);
// probe.hip
at::Tensor mfma_probe(const at::Tensor&, const at::Tensor&);
// lstm.hip
std::vector<at::Tensor> lstm_fwd(const at::Tensor&, const at::Tensor&,
                                 const at::Tensor&, bool, bool);
std::vector<at::Tensor> lstm_bwd(const at::Tensor&, const at::Tensor&,
                                 const at::Tensor&, const at::Tensor&,
                                 const at::Tensor&, const at::Tensor&, bool,
                                 bool);
std::vector<at::Tensor> bilstm_fwd_l(const at::Tensor&, const at::Tensor&,
                                     const at::Tensor&, bool, double);
at::Tensor bilstm_bwd_l(const at::Tensor&, const at::Tensor&,
                        const at::Tensor&, const at::Tensor&,
                        const at::Tensor&, bool, double);

PYBIND11_MODULE(_hip_ops, m) {
  m.doc() = "chinesener_amd gfx950 HIP kernels";
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("add_layernorm_fwd", &add_layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("bias_gelu_fwd", &bias_gelu_fwd);
  m.def("bias_gelu_bwd", &bias_gelu_bwd);
  m.def("masked_ce_fwd", &masked_ce_fwd);
  m.def("masked_ce_bwd", &masked_ce_bwd);
  m.def("colsum", &colsum);
  m.def("dropout_add_ln_fwd", &dropout_add_ln_fwd);
  m.def("mask_scale", &mask_scale);
  m.def("dropout_add_ln_bwd", &dropout_add_ln_bwd);
  m.def("bump_counter", &bump_counter);
  m.def("wgrad", &wgrad);
  m.def("wgrad2", &wgrad2);
  m.def("gemm_nt", &gemm_nt, py::arg("a"), py::arg("b"),
        py::arg("bias") = c10::nullopt, py::arg("fp32_out") = false);
  m.def("gemm_tn", &gemm_tn, py::arg("a"), py::arg("b"),
        py::arg("split") = 0, py::arg("fp32_out") = false);
  m.def("gemm_nn", &gemm_nn, py::arg("a"), py::arg("b"),
        py::arg("fp32_out") = false);
  m.def("gemm_nt_bias_gelu", &gemm_nt_bias_gelu, py::arg("a"), py::arg("b"),
        py::arg("bias"), py::arg("save_pre") = true);
  m.def("gemm_nn_dgelu", &gemm_nn_dgelu, py::arg("a"), py::arg("b"),
        py::arg("u"), py::arg("bias"));
  m.def("embed3_fwd", &embed3_fwd);
  m.def("embed3_bwd", &embed3_bwd, py::arg("dy"), py::arg("token_ids"),
        py::arg("segment_ids"), py::arg("V"), py::arg("P"), py::arg("S"));
  m.def("embed3_bwd_limits", &embed3_bwd_limits);
  m.def("crf_fwd", &crf_fwd);
  m.def("crf_pair_fwd", &crf_pair_fwd, py::arg("emissions"), py::arg("tags"),
        py::arg("lens"), py::arg("transitions"),
        py::arg("seqs_per_block") = 0);
  m.def("crf_fwd_route", &crf_fwd_route, py::arg("seq_len"),
        py::arg("label_size"));
  m.def("crf_grad_scale", &crf_grad_scale, py::arg("demis"),
        py::arg("dtrans"), py::arg("dll"));
  m.def("crf_viterbi", &crf_viterbi);
  m.def("crf_path_posterior", &crf_path_posterior, py::arg("emissions"),
        py::arg("lens"), py::arg("transitions"), py::arg("path"));
  m.def("crf_nbest", &crf_nbest, py::arg("emissions"), py::arg("lens"),
        py::arg("transitions"), py::arg("k"));
  m.def("crf_nbest_route", &crf_nbest_route, py::arg("seq_len"),
        py::arg("label_size"), py::arg("k"));
  m.def("crf_partial_fwd", &crf_partial_fwd, py::arg("emissions"),
        py::arg("allowed"), py::arg("lens"), py::arg("transitions"));
  m.def("crf_partial_route", &crf_partial_route, py::arg("seq_len"),
        py::arg("label_size"));
  m.def("crf_viterbi_constrained", &crf_viterbi_constrained,
        py::arg("emissions"), py::arg("allowed"), py::arg("lens"),
        py::arg("transitions"), py::arg("trans_allowed"));
  m.def("softlexicon_fwd", &softlexicon_fwd);
  m.def("softlexicon_bwd", &softlexicon_bwd);
  m.def("multi_tensor_adamw", &multi_tensor_adamw);
  m.def("multi_tensor_sumsq", &multi_tensor_sumsq);
  m.def("multi_tensor_scale", &multi_tensor_scale);
  m.def("adamw_build_meta", &adamw_build_meta);
  m.def("multi_tensor_adamw_run", &multi_tensor_adamw_run);
  m.def("norm_build_meta", &norm_build_meta);
  m.def("multi_tensor_sumsq_run", &multi_tensor_sumsq_run);
  m.def("multi_tensor_scale_run", &multi_tensor_scale_run);
  m.def("multi_tensor_adamw_tab_run", &multi_tensor_adamw_tab_run);
  m.def("sumsq_build_chunks", &sumsq_build_chunks);
  m.def("multi_tensor_sumsq_coef_run", &multi_tensor_sumsq_coef_run);
  m.def("grad_table_slots", &grad_table_slots);
  m.def("sumsq_chunk_elems", &sumsq_chunk_elems);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("attn_fwd_qkv", &attn_fwd_qkv);
  m.def("attn_bwd_qkv", &attn_bwd_qkv);
  m.def("attn_bwd_qkv_dbias", &attn_bwd_qkv_dbias);
  m.def("attn_tiled_fwd", &attn_tiled_fwd);
  m.def("attn_tiled_bwd", &attn_tiled_bwd);
  m.def("attn_tiled_fwd_qkv", &attn_tiled_fwd_qkv);
  m.def("attn_tiled_bwd_qkv", &attn_tiled_bwd_qkv);
  m.def("tener_attn_fwd", &tener_attn_fwd);
  m.def("tener_attn_bwd", &tener_attn_bwd);
  m.def("mfma_probe", &mfma_probe);
  m.def("lstm_fwd", &lstm_fwd);
  m.def("lstm_bwd", &lstm_bwd);
  m.def("bilstm_fwd", &bilstm_fwd_l);
  m.def("bilstm_bwd", &bilstm_bwd_l);
}
