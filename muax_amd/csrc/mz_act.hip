// mz_act.hip -- act() of the default MLP trio in one launch (mzs_act_mlp, mzs_act_mlp_host): the fused kernel's
// instances (mz_fused_g*.hip, the ones built on demand) and the wide-action kernel (mz_wide.hip).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "mz_handle.h"
#include "mz_fused_launch.h"
#include "mz_wide_launch.h"

using mzh::fail;

// Calls a dispatcher and, while it answers that its instance keeps the embeddings (kNeedEmbScratch: first launch without
// a tree export) or the root paths (kNeedPathScratch + words per node) in HBM and `p` has none: allocates them on the
// handle, patches `p` and calls again.  MZS_OK with the dispatcher's last answer in *rc, or the allocation's error.
// (wide_dispatch used to get one retry, for embeddings only: it never answers kNeedPathScratch nor asks twice -- same path)
template <class Call>
static int dispatch_with_scratch(mzs_handle* h, mz::FusedParams& p, int* rc, Call call) {
  const size_t BN = (size_t)h->cfg.batch * (h->cfg.num_simulations + 1);
  *rc = call();
  for (int tries = 0; tries < 2 && (*rc == mz::kNeedEmbScratch || *rc >= mz::kNeedPathScratch); ++tries) {
    if (*rc == mz::kNeedEmbScratch) {
      MZS_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->fused_emb), BN * h->cfg.embed_dim * sizeof(float)));
      p.emb_scratch = h->fused_emb;
    } else {
      const int words = *rc - mz::kNeedPathScratch;
      if (h->fused_path) MZS_HIP(h, hipFree(h->fused_path));
      h->fused_path = nullptr;
      h->fused_path_words = 0;
      MZS_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->fused_path), BN * words * sizeof(int32_t)));
      h->fused_path_words = words;
      p.path_scratch = h->fused_path;
      p.path_words = words;
    }
    *rc = call();
  }
  return MZS_OK;
}

extern "C" {

int mzs_act_mlp(mzs_handle* h, const mzs_act_args* a, void* stream_) {
  if (!h) return MZS_E_INVALID;
  if (!a || a->struct_size != (int32_t)sizeof(mzs_act_args))
    return fail(h, MZS_E_INVALID, "mzs_act_mlp: null or size mismatch (ABI)");
  if (!h->have_weights) return fail(h, MZS_E_INVALID, "mzs_act_mlp: call mzs_mlp_set_weights first");
  if (!a->obs || !a->action || !a->action_weights || !a->root_value)
    return fail(h, MZS_E_INVALID, "mzs_act_mlp: obs/action/action_weights/root_value must be set");
  const mzs_config& c = h->cfg;
  if (c.policy == 0 && !a->dirichlet_noise && a->dirichlet_fraction != 0.0f)
    return fail(h, MZS_E_INVALID, "mzs_act_mlp: dirichlet_fraction != 0 needs dirichlet_noise");
  if (c.num_simulations > mz::kMaxSims) {  // (the fused kernel's argument block holds 256 simulation keys)
    if (h->allow_generic) return mzh::act_mlp_generic(h, a, stream_);
    return fail(h, MZS_E_UNSUPPORTED, "mzs_act_mlp: no fused kernel instance for num_simulations > 256; use the generic route "
                                      "(mzs_mlp_allow_generic) or the step-wise path");
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MZS_HIP(h, hipSetDevice(c.device));

  mz::FusedParams p;
  memset(&p, 0, sizeof p);
  p.obs = a->obs; p.dirichlet_noise = a->dirichlet_noise; p.invalid = a->invalid_actions; p.gumbel = a->gumbel;
  const mzs_mlp_weights& w = h->w;
  mzh::copy_weights(w, p);
  p.action = a->action; p.action_weights = a->action_weights; p.root_value = a->root_value;
  p.search_value = a->search_value; p.depth_sum = a->depth_sum;
  if (a->tree) {
    const mzs_tree_view& t = *a->tree;
    const void* const* tp = reinterpret_cast<const void* const*>(&t);
    for (int i = 0; i < 12; ++i)
      if (!tp[i]) return fail(h, MZS_E_INVALID, "mzs_act_mlp: tree view has a null array");
    p.t_node_visits = t.node_visits; p.t_raw_values = t.raw_values; p.t_node_values = t.node_values;
    p.t_parents = t.parents; p.t_action_from_parent = t.action_from_parent;
    p.t_children_index = t.children_index; p.t_children_prior_logits = t.children_prior_logits;
    p.t_children_values = t.children_values; p.t_children_visits = t.children_visits;
    p.t_children_rewards = t.children_rewards; p.t_children_discounts = t.children_discounts;
    p.t_embeddings = t.embeddings;
    p.export_tree = 1;
  }
  p.B = c.batch; p.obs_dim = w.obs_dim; p.S = c.num_simulations; p.max_depth = c.max_depth;
  p.support = w.support_size; p.pred_on_parent = w.recurrent_pred_on;
  p.pb_c_init = c.pb_c_init; p.pb_c_base = c.pb_c_base;
  p.dirichlet_fraction = a->dirichlet_fraction; p.discount = w.discount; p.temperature = a->temperature;
  p.global_batch = (uint64_t)c.global_batch; p.root_offset = (uint64_t)c.root_offset;
  p.prof = h->prof;
  // (embeddings wider than 16 -- and those of every FusedCfg::LONG instance: long searches, wide action sets -- live in
  // HBM: the caller's export buffer when a tree is exported, else this scratch, allocated when a dispatcher asks for it)
  p.emb_scratch = p.export_tree ? nullptr : h->fused_emb;
  if (c.policy == 1) {
    // gumbel policy: seq_halving table on the device (once), root Gumbel key = split(key)[1]
    if (!h->fused_table) {
      const std::vector<int32_t> table = mzh::visit_table(c.max_num_considered_actions, c.num_simulations);
      MZS_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->fused_table), table.size() * sizeof(int32_t)));
      MZS_HIP(h, hipMemcpy(h->fused_table, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    p.visit_table = h->fused_table;
    p.max_considered = c.max_num_considered_actions;
    p.gumbel_scale = c.gumbel_scale;
    mzh::h_split(a->key, 2, 1, p.k_gumbel);
  }
  mzh::derive_keys(a->key, h->cfg.num_simulations, h->k_sample, h->sim_keys.data());
  p.k_sample[0] = h->k_sample[0]; p.k_sample[1] = h->k_sample[1];
  memcpy(p.sim_keys, h->sim_keys.data(), sizeof(uint32_t) * 2 * (size_t)c.num_simulations);  // <= kMaxSims (checked above)

  const int A = c.num_actions, E = c.embed_dim, F = 2 * w.support_size + 1, N = c.num_simulations + 1;
  p.F = F;
  const int mode = c.policy == 1 ? (c.qtransform == 1 ? 3 : 2) : (c.tiebreak ? 1 : 0);
  std::vector<mz::FusedDispatch> groups = {mz::fused_dispatch_g0, mz::fused_dispatch_g1, mz::fused_dispatch_g2,
                                           mz::fused_dispatch_g3, mz::fused_dispatch_g4};
  mz::jit_dispatchers(mode, &groups);  // instances built on demand (mzs_register_fused_dispatch[_muzero])
  // (tools/bench_generic.py: MZS_FORCE_GENERIC=1 sends a shape that HAS an instance through the generic route, for A/B timing)
  if (h->allow_generic && getenv("MZS_FORCE_GENERIC") != nullptr) return mzh::act_mlp_generic(h, a, stream_);
  // more 16-root workgroups than CUs: prefer a compact-record instance (two workgroups per CU), if the shape has one
  for (int compact = (c.batch > 16 * h->cu_count) ? 1 : 0; compact >= 0; --compact) {
    // (handed over whenever it exists: an instance for 128..255 simulations keeps its root paths there at any batch size)
    p.path_scratch = h->fused_path;
    p.path_words = h->fused_path_words;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      std::string err;
      int rc = 0;
      auto call = [&] { return groups[gi](mode, c.device, p, stream, A, E, F, N, compact != 0, &err); };
      if (int e = dispatch_with_scratch(h, p, &rc, call)) return e;
      if (rc == mz::kNoFusedInstance) continue;
      if (rc != MZS_OK) return fail(h, rc, "mzs_act_mlp: %s", err.c_str());
      return MZS_OK;
    }
  }
  // 17..64 actions: the lane-per-action kernel with the tree in LDS (mz_wide.cuh), each policy by its own opt-in
  if (mode >= 2 ? h->allow_wide_gumbel : h->allow_wide) {
    std::string err;
    int rc = 0;
    auto call = [&] { return mz::wide_dispatch(mode, h->allow_wide_gumbel, c.device, p, stream, A, E, F, &err); };
    if (int e = dispatch_with_scratch(h, p, &rc, call)) return e;
    if (rc == MZS_OK) return MZS_OK;
    if (rc != mz::kNoFusedInstance) return fail(h, rc, "mzs_act_mlp: %s", err.c_str());
  }
  if (h->allow_generic) return mzh::act_mlp_generic(h, a, stream_);
  return fail(h, MZS_E_UNSUPPORTED,
              "mzs_act_mlp: no fused kernel instance for this (A, E, F, S) (muax_amd/csrc/mz_instances.def); use the step-wise path");
}

int mzs_act_mlp_host(mzs_handle* h, const mzs_act_host_args* a, void* stream_) {
  if (!h) return MZS_E_INVALID;
  if (!a || a->struct_size != (int32_t)sizeof(mzs_act_host_args))
    return fail(h, MZS_E_INVALID, "mzs_act_mlp_host: null or size mismatch (ABI)");
  if (!h->have_weights) return fail(h, MZS_E_INVALID, "mzs_act_mlp_host: call mzs_mlp_set_weights first");
  if (!a->obs || !a->action || !a->action_weights || !a->root_value)
    return fail(h, MZS_E_INVALID, "mzs_act_mlp_host: obs/action/action_weights/root_value must be set");
  const mzs_config& c = h->cfg;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MZS_HIP(h, hipSetDevice(c.device));
  const size_t B = (size_t)c.batch, A = (size_t)c.num_actions, OD = (size_t)h->w.obs_dim;
  // staging layout (4-byte words): obs [B, OD] | noise [B, A] | invalid [B, A] bytes
  const size_t obs_b = B * OD * 4, noise_b = B * A * 4, inv_b = (B * A + 3) / 4 * 4, in_b = obs_b + noise_b + inv_b;
  const size_t out_b = B * (2 + A) * 4;
  if (h->host_in_bytes < in_b) {
    if (h->host_in) { hipHostFree(h->host_in); h->host_in = nullptr; }
    MZS_HIP(h, hipHostMalloc(&h->host_in, in_b, hipHostMallocDefault));
    h->host_in_bytes = in_b;
  }
  if (!h->host_out) MZS_HIP(h, hipHostMalloc(&h->host_out, out_b, hipHostMallocDefault));
  if (!h->dev_noise) MZS_HIP(h, hipMalloc(&h->dev_noise, noise_b));
  // The kernels read the host's inputs and write its outputs THROUGH THE PINNED STAGING BUFFERS themselves (hipHostMalloc
  // memory is mapped into the device's address space, coherent): an act moves 16..32 bytes per root each way, read once
  // at the kernel's start and written once at its end, and a copy command costs more in launch and engine latency than
  // those bytes cost over the host link.  Only the drawn root noise lives in device memory (its producer is a kernel).
  char* hin = static_cast<char*>(h->host_in);
  char* hin_dev = nullptr;
  float* hout_dev = nullptr;
  MZS_HIP(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&hin_dev), h->host_in, 0));
  MZS_HIP(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&hout_dev), h->host_out, 0));
  const bool muzero = c.policy == 0;
  const bool given = muzero && a->dirichlet_noise != nullptr;
  const bool draw = muzero && !given && a->draw_dirichlet != 0 && a->dirichlet_fraction != 0.0f;
  float* d_noise = static_cast<float*>(h->dev_noise);
  if (draw) {  // first: it needs nothing from the host and runs while the host fills the staging buffer
    uint32_t kd[2];
    mzh::h_split(a->key, 3, 1, kd);  // mctx: rng_key, dirichlet_rng_key, search_rng_key = split(rng_key, 3)
    if (int rc = mzs_dirichlet(c.device, kd, a->dirichlet_alpha, c.batch, c.num_actions, c.global_batch, c.root_offset,
                               d_noise, stream_))
      return fail(h, rc, "mzs_act_mlp_host: %s", mzs_last_error(nullptr));
  }
  memcpy(hin, a->obs, obs_b);
  if (given) memcpy(hin + obs_b, a->dirichlet_noise, noise_b);
  if (a->invalid_actions) memcpy(hin + obs_b + noise_b, a->invalid_actions, B * A);
  float* dout = hout_dev;
  mzs_act_args args;
  memset(&args, 0, sizeof args);
  args.struct_size = (int32_t)sizeof args;
  args.obs = reinterpret_cast<const float*>(hin_dev);
  args.dirichlet_noise = draw ? d_noise : (given ? reinterpret_cast<const float*>(hin_dev + obs_b) : nullptr);
  args.invalid_actions = a->invalid_actions ? reinterpret_cast<const uint8_t*>(hin_dev + obs_b + noise_b) : nullptr;
  args.key[0] = a->key[0]; args.key[1] = a->key[1];
  args.dirichlet_fraction = (given || draw) ? a->dirichlet_fraction : 0.0f;
  args.temperature = a->temperature;
  args.action = reinterpret_cast<int32_t*>(dout);
  args.action_weights = dout + B;
  args.root_value = dout + B + B * A;
  if (int rc = mzs_act_mlp(h, &args, stream_)) return rc;
  MZS_HIP(h, hipStreamSynchronize(stream));
  const char* hout = static_cast<const char*>(h->host_out);
  memcpy(a->action, hout, B * 4);
  memcpy(a->action_weights, hout + B * 4, B * A * 4);
  memcpy(a->root_value, hout + B * 4 + B * A * 4, B * 4);
  return MZS_OK;
}

#ifdef MZ_PROFILE
// tools-only entry point (not part of the ABI): per-wave phase cycle counters [waves][8]
int mzs_debug_profile(mzs_handle* h, uint64_t* device_buffer) {
  if (!h) return MZS_E_INVALID;
  h->prof = device_buffer;
  return MZS_OK;
}
#endif

}  // extern "C"
