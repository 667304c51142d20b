// pybind bindings for the lingvo_amd gfx950 HIP op library.
#include <torch/extension.h>

#include <vector>

// layer_norm.hip
std::vector<torch::Tensor> layer_norm_fwd(torch::Tensor x,
                                          torch::Tensor scale,
                                          torch::Tensor bias, double eps,
                                          bool rms);
std::vector<torch::Tensor> layer_norm_bwd(torch::Tensor dy, torch::Tensor x,
                                          torch::Tensor scale,
                                          torch::Tensor mean,
                                          torch::Tensor rstd, bool rms,
                                          c10::optional<torch::Tensor> dres);

// mfma_probe.hip
torch::Tensor mfma_probe(torch::Tensor a, torch::Tensor bT);
torch::Tensor tr16_probe(torch::Tensor a, torch::Tensor b);

// flash_attn.hip
std::vector<torch::Tensor> fa_fwd(torch::Tensor q, torch::Tensor k,
                                  torch::Tensor v,
                                  c10::optional<torch::Tensor> klen,
                                  c10::optional<torch::Tensor> bias,
                                  c10::optional<torch::Tensor> qseg,
                                  c10::optional<torch::Tensor> kseg,
                                  int64_t win_l, int64_t win_r,
                                  int64_t bias_clip, double scale,
                                  int64_t chunk_size, int64_t left_chunks);
std::vector<torch::Tensor> fa_bwd(torch::Tensor dout, torch::Tensor q,
                                  torch::Tensor k, torch::Tensor v,
                                  torch::Tensor o, torch::Tensor lse,
                                  c10::optional<torch::Tensor> klen,
                                  c10::optional<torch::Tensor> bias,
                                  c10::optional<torch::Tensor> qseg,
                                  c10::optional<torch::Tensor> kseg,
                                  bool bias_grad, int64_t win_l,
                                  int64_t win_r, int64_t bias_clip,
                                  double scale, int64_t chunk_size,
                                  int64_t left_chunks,
                                  c10::optional<torch::Tensor> dq_out,
                                  c10::optional<torch::Tensor> dk_out,
                                  c10::optional<torch::Tensor> dv_out,
                                  const std::string& route);

// conv1d.hip
torch::Tensor dwconv1d_fwd(torch::Tensor x, torch::Tensor w,
                           c10::optional<torch::Tensor> bias, int64_t pad,
                           const std::string& route,
                           c10::optional<torch::Tensor> y_out);
std::vector<torch::Tensor> dwconv1d_bwd(
    torch::Tensor dy, torch::Tensor x, torch::Tensor w, int64_t pad,
    const std::string& route, c10::optional<torch::Tensor> dx_out,
    c10::optional<torch::Tensor> dw_out, c10::optional<torch::Tensor> db_out);
torch::Tensor glu_dwconv1d_fwd(torch::Tensor h,
                               c10::optional<torch::Tensor> paddings,
                               torch::Tensor w,
                               c10::optional<torch::Tensor> bias, int64_t pad,
                               const std::string& route,
                               c10::optional<torch::Tensor> y_out);
std::vector<torch::Tensor> glu_dwconv1d_bwd(
    torch::Tensor dy, torch::Tensor h, c10::optional<torch::Tensor> paddings,
    torch::Tensor w, int64_t pad, const std::string& route,
    c10::optional<torch::Tensor> dh_out, c10::optional<torch::Tensor> dw_out,
    c10::optional<torch::Tensor> db_out,
    c10::optional<torch::Tensor> dcol_out);

// dwconv_tiled.hip
int64_t dwconv_tile_len();

// softmax_xent.hip
std::vector<torch::Tensor> xent_fwd(torch::Tensor logits,
                                    torch::Tensor labels);
torch::Tensor xent_bwd(torch::Tensor logits, torch::Tensor labels,
                       torch::Tensor lse, torch::Tensor gout);

// dropout.hip
torch::Tensor dropout_fwd(torch::Tensor x, c10::optional<torch::Tensor> res,
                          int64_t seed,
                          c10::optional<torch::Tensor> step_seed,
                          double keep, int64_t act, double scale,
                          c10::optional<torch::Tensor> pad, int64_t d);
torch::Tensor dropout_bwd(torch::Tensor dy, c10::optional<torch::Tensor> x,
                          int64_t seed,
                          c10::optional<torch::Tensor> step_seed,
                          double keep, int64_t act, double scale,
                          c10::optional<torch::Tensor> pad, int64_t d);
std::vector<torch::Tensor> dropout_bwd_colsum(
    torch::Tensor dy, c10::optional<torch::Tensor> x, int64_t seed,
    c10::optional<torch::Tensor> step_seed, double keep, int64_t act,
    double scale, c10::optional<torch::Tensor> pad, int64_t d);

// group_norm.hip
std::vector<torch::Tensor> group_norm_fwd(torch::Tensor x,
                                          torch::Tensor gamma,
                                          torch::Tensor beta,
                                          c10::optional<torch::Tensor> pad,
                                          int64_t groups, double eps,
                                          int64_t act,
                                          const std::string& route);
std::vector<torch::Tensor> group_norm_bwd(torch::Tensor dy, torch::Tensor x,
                                          torch::Tensor gamma,
                                          torch::Tensor beta,
                                          c10::optional<torch::Tensor> pad,
                                          torch::Tensor mean,
                                          torch::Tensor rstd,
                                          int64_t groups, int64_t act);

// lstm_gates.hip
std::vector<torch::Tensor> lstm_gates_fwd_op(torch::Tensor gates,
                                             torch::Tensor c0, double fgb,
                                             double cap);
std::vector<torch::Tensor> lstm_gates_bwd_op(
    torch::Tensor gates, torch::Tensor c0, torch::Tensor c1,
    torch::Tensor dm1, c10::optional<torch::Tensor> dc1, double fgb,
    double cap);

// input_pipeline.cpp
void RegisterInputPipeline(py::module_& m);

// wpm_tokenizer.cpp
void RegisterWpmTokenizer(py::module_& m);

// record_batcher.cpp
void RegisterRecordBatcher(py::module_& m);

// embedding.hip
torch::Tensor emb_gather(torch::Tensor table, torch::Tensor ids,
                         double scale);
torch::Tensor emb_scatter_add(torch::Tensor dy, torch::Tensor ids,
                              int64_t vocab, double scale);

// moe_gating.hip
std::vector<torch::Tensor> moe_positions(torch::Tensor top1,
                                         torch::Tensor top2,
                                         int64_t num_experts);

// s2d.hip
torch::Tensor s2d_fwd(torch::Tensor x);
torch::Tensor s2d_inv(torch::Tensor dX, int64_t C);
torch::Tensor pad_scatter(torch::Tensor dout);
torch::Tensor conv1_s2d_fwd(torch::Tensor x, torch::Tensor w1,
                            torch::Tensor b1, int64_t max_blocks);
std::vector<torch::Tensor> conv1_s2d_bwd(torch::Tensor dX, torch::Tensor X,
                                         torch::Tensor x, int64_t max_blocks);
torch::Tensor unpad_relu(torch::Tensor O);
std::vector<torch::Tensor> pad_scatter_relu_bwd(torch::Tensor dout,
                                                torch::Tensor y,
                                                int64_t max_blocks);

// topk.hip
std::vector<torch::Tensor> topk_rows(torch::Tensor scores, int64_t k);

// las_decoder.hip
void smallm_gemm(torch::Tensor a, torch::Tensor wt,
                 c10::optional<torch::Tensor> pre, torch::Tensor out,
                 int64_t k, int64_t wt_col0, double alpha,
                 int64_t pre_mode);
std::vector<torch::Tensor> attend_fwd(torch::Tensor q, torch::Tensor enc,
                                      torch::Tensor pad, double scale);
std::vector<torch::Tensor> attend_bwd(torch::Tensor dctx,
                                      torch::Tensor probs, torch::Tensor q,
                                      torch::Tensor enc, torch::Tensor denc,
                                      double scale);
void attend_step_fwd(torch::Tensor q, torch::Tensor enc, torch::Tensor pad,
                     double scale, torch::Tensor probs, torch::Tensor ctx,
                     torch::Tensor ctx32, int64_t variant);
void attend_step_bwd(torch::Tensor dctx_a, c10::optional<torch::Tensor> dctx_b,
                     torch::Tensor probs, torch::Tensor ctx32,
                     torch::Tensor enc, double scale, torch::Tensor dctx_out,
                     torch::Tensor dl, torch::Tensor dq, int64_t variant);
void attend_denc(torch::Tensor dl, torch::Tensor probs, torch::Tensor qs,
                 torch::Tensor dctx, torch::Tensor out);
int64_t attend_step_lds_bytes(int64_t s, int64_t d, bool bwd,
                              int64_t variant);
int64_t attend_denc_row_tile();
int64_t attend_lds_limit();
int64_t attend_lds_bytes(int64_t s, int64_t d, bool bwd);

// las_step.hip
void las_step_fwd(c10::optional<torch::Tensor> a1,
                  c10::optional<torch::Tensor> a2, torch::Tensor wt,
                  torch::Tensor pre, c10::optional<torch::Tensor> c_prev,
                  torch::Tensor gates, torch::Tensor c_out,
                  torch::Tensor m_out, double fgb, double cap,
                  int64_t rows_per_block);
void las_cell_bwd(torch::Tensor a, torch::Tensor wt,
                  c10::optional<torch::Tensor> add_b,
                  c10::optional<torch::Tensor> add_f, torch::Tensor gates,
                  c10::optional<torch::Tensor> c_prev, torch::Tensor dc_carry,
                  bool has_dc, torch::Tensor dgates,
                  c10::optional<torch::Tensor> pass_out, double fgb,
                  double cap, int64_t rows_per_block);

// lstm_scan.hip
void lstm_scan_fwd(torch::Tensor gates, torch::Tensor c, torch::Tensor m,
                   torch::Tensor pad, torch::Tensor wmt, int64_t rev_mask,
                   double fgb, double cap, int64_t s_begin, int64_t s_end,
                   int64_t rows_per_block);
void lstm_scan_bwd(torch::Tensor gates, torch::Tensor c, torch::Tensor pad,
                   torch::Tensor wm, c10::optional<torch::Tensor> dm_out,
                   c10::optional<torch::Tensor> dc_out,
                   torch::Tensor dgates, torch::Tensor dc_carry,
                   torch::Tensor dm_pass, int64_t rev_mask, double fgb,
                   double cap, int64_t s_begin, int64_t s_end,
                   int64_t rows_per_block);

// ctc.hip
std::vector<torch::Tensor> ctc_fwd(torch::Tensor logits,
                                   torch::Tensor logit_lengths,
                                   torch::Tensor labels,
                                   torch::Tensor label_lengths,
                                   int64_t blank);
torch::Tensor ctc_bwd(torch::Tensor logits, torch::Tensor logit_lengths,
                      torch::Tensor labels, torch::Tensor label_lengths,
                      torch::Tensor lse, torch::Tensor emis,
                      torch::Tensor alpha, torch::Tensor beta,
                      torch::Tensor nll, torch::Tensor valid,
                      torch::Tensor gout, int64_t blank);
int64_t ctc_max_label_len();
std::vector<torch::Tensor> ctc_align(torch::Tensor logits,
                                     torch::Tensor logit_lengths,
                                     torch::Tensor labels,
                                     torch::Tensor label_lengths,
                                     int64_t blank, bool lds_masks);

// rnnt.hip
std::vector<torch::Tensor> rnnt_fwd(torch::Tensor logits,
                                    torch::Tensor logit_lengths,
                                    torch::Tensor labels,
                                    torch::Tensor label_lengths,
                                    int64_t blank);
torch::Tensor rnnt_bwd(torch::Tensor logits, torch::Tensor logit_lengths,
                       torch::Tensor labels, torch::Tensor label_lengths,
                       torch::Tensor lse, torch::Tensor emis,
                       torch::Tensor alpha, torch::Tensor beta,
                       torch::Tensor valid, torch::Tensor gnll,
                       int64_t blank);
int64_t rnnt_max_label_len();

// attn_decode.hip
torch::Tensor attn_decode(torch::Tensor q, torch::Tensor key_cache,
                          torch::Tensor value_cache,
                          c10::optional<torch::Tensor> q_start_t,
                          int64_t q_start,
                          c10::optional<torch::Tensor> bias, int64_t win_l,
                          int64_t bias_clip, double scale,
                          int64_t num_splits);
int64_t attn_decode_num_splits(int64_t B, int64_t NKV, int64_t keys,
                               int64_t rows);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  RegisterInputPipeline(m);
  RegisterWpmTokenizer(m);
  RegisterRecordBatcher(m);
  m.def("group_norm_fwd", &group_norm_fwd, "Fused padded GroupNorm fwd",
        py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("pad"),
        py::arg("groups"), py::arg("eps"), py::arg("act"),
        py::arg("route") = "auto");
  m.def("group_norm_bwd", &group_norm_bwd, "Fused padded GroupNorm bwd");
  m.def("lstm_gates_fwd", &lstm_gates_fwd_op, "Fused LSTM gates fwd");
  m.def("lstm_gates_bwd", &lstm_gates_bwd_op, "Fused LSTM gates bwd");
  m.def("dropout_fwd", &dropout_fwd, "Fused dropout fwd");
  m.def("dropout_bwd", &dropout_bwd, "Fused dropout bwd");
  m.def("dropout_bwd_colsum", &dropout_bwd_colsum,
        "Fused dropout bwd + fp32 column sums of dx");
  m.def("xent_fwd", &xent_fwd, "Fused softmax-xent fwd");
  m.def("xent_bwd", &xent_bwd, "Fused softmax-xent bwd");
  m.def("dwconv1d_fwd", &dwconv1d_fwd, "Depthwise time conv fwd",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("pad"),
        py::arg("route") = "auto", py::arg("y_out") = py::none());
  m.def("dwconv1d_bwd", &dwconv1d_bwd, "Depthwise time conv bwd",
        py::arg("dy"), py::arg("x"), py::arg("w"), py::arg("pad"),
        py::arg("route") = "auto", py::arg("dx_out") = py::none(),
        py::arg("dw_out") = py::none(), py::arg("db_out") = py::none());
  m.def("glu_dwconv1d_fwd", &glu_dwconv1d_fwd,
        "conv(mask * glu(h)) + bias in one kernel", py::arg("h"),
        py::arg("paddings"), py::arg("w"), py::arg("bias"), py::arg("pad"),
        py::arg("route") = "auto", py::arg("y_out") = py::none());
  m.def("glu_dwconv1d_bwd", &glu_dwconv1d_bwd,
        "dh, dw, db and the fp32 column sums of dh of glu_dwconv1d_fwd",
        py::arg("dy"), py::arg("h"), py::arg("paddings"), py::arg("w"),
        py::arg("pad"), py::arg("route") = "auto",
        py::arg("dh_out") = py::none(), py::arg("dw_out") = py::none(),
        py::arg("db_out") = py::none(), py::arg("dcol_out") = py::none());
  m.def("dwconv_tile_len", &dwconv_tile_len,
        "Time rows per tile of the tiled depthwise convolution");
  m.def("layer_norm_fwd", &layer_norm_fwd, "Fused LayerNorm/RMSNorm fwd");
  m.def("layer_norm_bwd", &layer_norm_bwd, "Fused LayerNorm/RMSNorm bwd",
        py::arg("dy"), py::arg("x"), py::arg("scale"), py::arg("mean"),
        py::arg("rstd"), py::arg("rms"), py::arg("dres") = py::none());
  m.def("mfma_probe", &mfma_probe, "MFMA 16x16x32 layout probe");
  m.def("tr16_probe", &tr16_probe, "ds_read_tr16_b64 layout probe");
  m.def("fa_fwd", &fa_fwd, "Flash attention forward");
  m.def("fa_bwd", &fa_bwd, "Flash attention backward", py::arg("dout"),
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("lse"), py::arg("klen"), py::arg("bias"), py::arg("qseg"),
        py::arg("kseg"), py::arg("bias_grad"), py::arg("win_l"),
        py::arg("win_r"), py::arg("bias_clip"), py::arg("scale"),
        py::arg("chunk_size"), py::arg("left_chunks"),
        py::arg("dq_out") = py::none(), py::arg("dk_out") = py::none(),
        py::arg("dv_out") = py::none(), py::arg("route") = "auto");
  m.def("emb_gather", &emb_gather, "Embedding gather fwd");
  m.def("emb_scatter_add", &emb_scatter_add,
        "Deterministic embedding scatter-add bwd");
  m.def("moe_positions", &moe_positions,
        "Deterministic MoE top-2 position scan");
  m.def("smallm_gemm", &smallm_gemm,
        "Small-M MFMA GEMM (decode-step projections)");
  m.def("attend_fwd", &attend_fwd, "Fused dot-attention step fwd");
  m.def("attend_bwd", &attend_bwd, "Fused dot-attention step bwd");
  m.def("attend_step_fwd", &attend_step_fwd,
        "One-pass dot-attention step fwd into caller rows (probs, ctx, ctx32)",
        py::arg("q"), py::arg("enc"), py::arg("pad"), py::arg("scale"),
        py::arg("probs"), py::arg("ctx"), py::arg("ctx32"),
        py::arg("variant") = 0);
  m.def("attend_step_bwd", &attend_step_bwd,
        "One-pass dot-attention step bwd without dEnc (dctx, dl, dq out)",
        py::arg("dctx_a"), py::arg("dctx_b"), py::arg("probs"),
        py::arg("ctx32"), py::arg("enc"), py::arg("scale"),
        py::arg("dctx_out"), py::arg("dl"), py::arg("dq"),
        py::arg("variant") = 0);
  m.def("attend_denc", &attend_denc,
        "dEnc of the whole recurrence from the stacked dl, probs, q, dctx");
  m.def("attend_step_lds_bytes", &attend_step_lds_bytes,
        "Dynamic LDS bytes attend_step_fwd/bwd ask for at (S, D, variant)");
  m.def("attend_denc_row_tile", &attend_denc_row_tile,
        "Rows of S one attend_denc workgroup owns");
  m.def("attend_lds_limit", &attend_lds_limit,
        "Dynamic LDS bytes an attend_* launch may ask for on this device");
  m.def("attend_lds_bytes", &attend_lds_bytes,
        "Dynamic LDS bytes attend_fwd/attend_bwd ask for at (S, D)");
  m.def("las_step_fwd", &las_step_fwd,
        "Decoder LSTM stage fwd: two-source step GEMM with the cell as "
        "epilogue, into caller rows (gates, c, m)",
        py::arg("a1"), py::arg("a2"), py::arg("wt"), py::arg("pre"),
        py::arg("c_prev"), py::arg("gates"), py::arg("c_out"),
        py::arg("m_out"), py::arg("fgb"), py::arg("cap"),
        py::arg("rows_per_block") = 0);
  m.def("las_cell_bwd", &las_cell_bwd,
        "Decoder LSTM cell bwd with its data-gradient GEMM as prologue "
        "(dgates out, fp32 dc_carry in place, optional fp32 pass_out half)",
        py::arg("a"), py::arg("wt"), py::arg("add_b"), py::arg("add_f"),
        py::arg("gates"), py::arg("c_prev"), py::arg("dc_carry"),
        py::arg("has_dc"), py::arg("dgates"), py::arg("pass_out"),
        py::arg("fgb"), py::arg("cap"), py::arg("rows_per_block") = 0);
  m.def("lstm_scan_fwd", &lstm_scan_fwd,
        "Fused LSTM scan forward: one launch per step, all directions");
  m.def("lstm_scan_bwd", &lstm_scan_bwd,
        "Fused LSTM scan backward: one launch per step, all directions");
  m.def("ctc_fwd", &ctc_fwd,
        "CTC loss forward: nll, valid and the backward's workspaces");
  m.def("ctc_bwd", &ctc_bwd, "CTC loss backward: dlogits");
  m.def("ctc_max_label_len", &ctc_max_label_len,
        "Largest label width L the CTC kernels support");
  m.def("ctc_align", &ctc_align,
        "CTC forced alignment: frame ids, token spans and log-probs, score, "
        "valid");
  m.def("rnnt_fwd", &rnnt_fwd,
        "Transducer loss forward: nll, valid and the backward's workspaces");
  m.def("rnnt_bwd", &rnnt_bwd, "Transducer loss backward: dlogits");
  m.def("rnnt_max_label_len", &rnnt_max_label_len,
        "Largest label width U the transducer kernels support");
  m.def("attn_decode", &attn_decode,
        "KV-cache attention (ExtendStep/StreamStep): split-K decode kernel "
        "+ combine",
        py::arg("q"), py::arg("key_cache"), py::arg("value_cache"),
        py::arg("q_start_t"), py::arg("q_start"), py::arg("bias"),
        py::arg("win_l"), py::arg("bias_clip"), py::arg("scale"),
        py::arg("num_splits") = 0);
  m.def("attn_decode_num_splits", &attn_decode_num_splits,
        "Split count attn_decode picks for (B, NKV, keys, rows = C * N/NKV)",
        py::arg("B"), py::arg("NKV"), py::arg("keys"), py::arg("rows") = 1);
  m.def("s2d_fwd", &s2d_fwd, "Space-to-depth + pad (conv frontend)");
  m.def("topk_rows", &topk_rows, "Row-wise top-k (beam pruning, K12)");
  m.def("s2d_inv", &s2d_inv, "Inverse space-to-depth");
  m.def("pad_scatter", &pad_scatter, "Zero-border pad scatter");
  m.def("conv1_s2d_fwd", &conv1_s2d_fwd,
        "relu(conv1(x) + b1) (Cin=1, 3x3/s2) written in padded s2d layout",
        py::arg("x"), py::arg("w1"), py::arg("b1"), py::arg("max_blocks") = 0);
  m.def("conv1_s2d_bwd", &conv1_s2d_bwd,
        "conv1 weight and bias gradients (fp32) from dX and X in s2d layout",
        py::arg("dX"), py::arg("X"), py::arg("x"), py::arg("max_blocks") = 0);
  m.def("unpad_relu", &unpad_relu, "relu(O[:, 1:, 1:, :]), contiguous");
  m.def("pad_scatter_relu_bwd", &pad_scatter_relu_bwd,
        "Zero-border pad of dout * (y > 0) plus its fp32 column sums",
        py::arg("dout"), py::arg("y"), py::arg("max_blocks") = 0);
}
