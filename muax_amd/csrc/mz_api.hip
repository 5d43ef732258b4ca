// mz_api.hip -- host side of the C-ABI (include/mzsearch.h): the handle's lifetime, weights and opt-ins, the error slots, the
// registries of on-demand instances; routes: mz_act / mz_stepwise / mz_train / mz_selftest .hip.  Pure HIP runtime, no torch.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>

#include "mz_handle.h"
#include "mz_fused_launch.h"

namespace {

thread_local std::string g_create_error;  // message of the last failure of an entry point without a handle

// fused-kernel instances built on demand and registered at run time (mzs_register_fused_dispatch; muax_amd/_jit.py)
std::mutex g_jit_mutex;
std::vector<mz::FusedDispatch> g_jit_dispatch;
std::vector<mz::FusedDispatch> g_jit_dispatch_muzero;  // MuZero-policy-only instances: tried before the all-modes ones
// training-step instances built on demand (mz_train_jit.hip): launcher of one (A, E, F = 2 support + 1) each
struct JitTrain { int A, E, F; mzh::JitTrainLaunch launch; };
std::vector<JitTrain> g_jit_train;
// ... of the stochastic family (mz_stoch_train_jit.hip): one (A, C, E, F) at one observation cap each
struct JitStochTrain { int A, C, E, F, OB; mzh::JitTrainLaunch launch; };
std::vector<JitStochTrain> g_jit_stoch_train;

}  // namespace

int mzh::fail(mzs_handle* h, int code, const char* fmt, const char* a) {
  char buf[512];
  snprintf(buf, sizeof buf, fmt, a);
  if (h) h->err = buf; else g_create_error = buf;
  return code;
}
mzh::JitTrainLaunch mzh::jit_train_instance(int A, int E, int F) {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  for (const JitTrain& t : g_jit_train)
    if (t.A == A && t.E == E && t.F == F) return t.launch;
  return nullptr;
}
mzh::JitTrainLaunch mzh::jit_stochastic_train_instance(int A, int C, int E, int F, int obs_dim) {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  const JitStochTrain* best = nullptr;
  for (const JitStochTrain& t : g_jit_stoch_train)
    if (t.A == A && t.C == C && t.E == E && t.F == F && obs_dim >= 1 && obs_dim <= t.OB && (!best || t.OB < best->OB)) best = &t;
  return best ? best->launch : nullptr;
}
void mz::jit_dispatchers(int mode, std::vector<FusedDispatch>* out) {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  if (mode < 2) out->insert(out->end(), g_jit_dispatch_muzero.begin(), g_jit_dispatch_muzero.end());
  out->insert(out->end(), g_jit_dispatch.begin(), g_jit_dispatch.end());
}
using mzh::fail;

extern "C" {

int mzs_abi_version(void) { return MZS_ABI_VERSION; }
int mzs_fused_jit_abi(void) { return MZS_ABI_VERSION * 1000 + (int)(sizeof(mz::FusedParams) % 1000); }

int mzs_register_train_dispatch(void* launch, int32_t num_actions, int32_t embed_dim, int32_t full_support, int32_t jit_abi) {
  if (!launch) return fail(nullptr, MZS_E_INVALID, "mzs_register_train_dispatch: null");
  if (jit_abi != mzs_train_jit_abi())
    return fail(nullptr, MZS_E_INVALID, "mzs_register_train_dispatch: the side library was built from other sources (ABI)");
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  for (const JitTrain& t : g_jit_train)
    if (t.A == num_actions && t.E == embed_dim && t.F == full_support) return MZS_OK;
  g_jit_train.push_back({num_actions, embed_dim, full_support, reinterpret_cast<mzh::JitTrainLaunch>(launch)});
  return MZS_OK;
}

int mzs_register_stochastic_train_dispatch(void* launch, int32_t num_actions, int32_t num_chance_outcomes, int32_t embed_dim,
                                           int32_t full_support, int32_t obs_cap, int32_t jit_abi) {
  if (!launch) return fail(nullptr, MZS_E_INVALID, "mzs_register_stochastic_train_dispatch: null");
  if (jit_abi != mzs_stochastic_train_jit_abi())
    return fail(nullptr, MZS_E_INVALID,
                "mzs_register_stochastic_train_dispatch: the side library was built from other sources (ABI)");
  if (obs_cap != 32 && obs_cap != 64 && obs_cap != 96 && obs_cap != 128)
    return fail(nullptr, MZS_E_INVALID, "mzs_register_stochastic_train_dispatch: obs_cap must be 32, 64, 96 or 128");
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  for (const JitStochTrain& t : g_jit_stoch_train)
    if (t.A == num_actions && t.C == num_chance_outcomes && t.E == embed_dim && t.F == full_support && t.OB == obs_cap)
      return MZS_OK;
  g_jit_stoch_train.push_back({num_actions, num_chance_outcomes, embed_dim, full_support, obs_cap,
                               reinterpret_cast<mzh::JitTrainLaunch>(launch)});
  return MZS_OK;
}

const char* mzs_last_error(const mzs_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int mzs_create(const mzs_config* cfg, mzs_handle** out) {
  if (!cfg || !out) return fail(nullptr, MZS_E_INVALID, "mzs_create: null argument");
  if (cfg->struct_size != (int32_t)sizeof(mzs_config))
    return fail(nullptr, MZS_E_INVALID, "mzs_create: mzs_config size mismatch (ABI)");
  if (cfg->batch <= 0 || cfg->num_actions <= 0 || cfg->num_simulations <= 0 || cfg->embed_dim <= 0)
    return fail(nullptr, MZS_E_INVALID, "mzs_create: batch, num_actions, num_simulations, embed_dim must be positive");
  if (cfg->num_actions > 64) return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_create: num_actions > 64");
  if (cfg->num_simulations >= 65535) return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_create: num_simulations too large");
  if (cfg->policy < 0 || cfg->policy > 2)
    return fail(nullptr, MZS_E_INVALID, "mzs_create: policy must be 0 (muzero), 1 (gumbel) or 2 (stochastic)");
  if (cfg->policy == 2) {
    const int es = cfg->state_embed_dim > 0 ? cfg->state_embed_dim : cfg->embed_dim;
    const int ea = cfg->afterstate_embed_dim > 0 ? cfg->afterstate_embed_dim : cfg->embed_dim;
    if (cfg->num_chance_outcomes <= 0) return fail(nullptr, MZS_E_INVALID, "mzs_create: the stochastic policy needs num_chance_outcomes > 0");
    if (cfg->num_actions + cfg->num_chance_outcomes > 64)
      return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_create: num_actions + num_chance_outcomes > 64");
    if (cfg->embed_dim != (es > ea ? es : ea))
      return fail(nullptr, MZS_E_INVALID, "mzs_create: embed_dim must be max(state_embed_dim, afterstate_embed_dim)");
    if (cfg->embed_dim >= mz::kWideEmb)
      return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_create: the stochastic policy takes embeddings narrower than 256 floats");
    static_assert(mz::kWideEmb == 256, "the message above names the bound");
  } else if (cfg->num_chance_outcomes != 0) {
    return fail(nullptr, MZS_E_INVALID, "mzs_create: num_chance_outcomes is for policy 2 (stochastic) only");
  }
  if (cfg->qtransform != 0 && !(cfg->qtransform == 1 && cfg->policy == 1))
    return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_create: qtransform_completed_by_mix_value is built for the gumbel policy only");
  if (cfg->policy == 1 && cfg->max_num_considered_actions < 0)
    return fail(nullptr, MZS_E_INVALID, "mzs_create: max_num_considered_actions");
  if (int rc = mzh::check_device(cfg->device, "mzs_create")) return rc;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
    return fail(nullptr, MZS_E_RUNTIME, "mzs_create: hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, MZS_E_NODEVICE, "mzs_create: device is %s, kernels are built for gfx950 only", prop.gcnArchName);
  mzs_handle* h = new mzs_handle();
  h->cfg = *cfg;
  h->cu_count = prop.multiProcessorCount;
  if (h->cfg.global_batch <= 0) h->cfg.global_batch = cfg->batch;
  if (h->cfg.state_embed_dim <= 0) h->cfg.state_embed_dim = cfg->embed_dim;
  if (h->cfg.afterstate_embed_dim <= 0) h->cfg.afterstate_embed_dim = cfg->embed_dim;
  if (h->cfg.root_offset < 0 || h->cfg.root_offset + cfg->batch > h->cfg.global_batch) {
    delete h;
    return fail(nullptr, MZS_E_INVALID, "mzs_create: root_offset + batch exceeds global_batch");
  }
  memset(&h->w, 0, sizeof h->w);
  h->sim_keys.assign(2 * (size_t)cfg->num_simulations, 0u);
  *out = h;
  return MZS_OK;
}

int mzs_mlp_allow_generic(mzs_handle* h, int32_t allow) {
  if (!h) return MZS_E_INVALID;
  h->allow_generic = allow != 0;
  return MZS_OK;
}
int mzs_mlp_allow_wide(mzs_handle* h, int32_t allow) {
  if (!h) return MZS_E_INVALID;
  h->allow_wide = allow != 0;
  return MZS_OK;
}
int mzs_mlp_allow_wide_gumbel(mzs_handle* h, int32_t allow) {
  if (!h) return MZS_E_INVALID;
  h->allow_wide_gumbel = allow != 0;
  return MZS_OK;
}

int mzs_destroy(mzs_handle* h) {
  if (!h) return MZS_OK;
  hipSetDevice(h->cfg.device);
  h->step.release();
  if (h->fused_table) hipFree(h->fused_table);
  if (h->fused_emb) hipFree(h->fused_emb);
  if (h->fused_path) hipFree(h->fused_path);
  if (h->jump_slab) hipFree(h->jump_slab);
  if (h->host_in) hipHostFree(h->host_in);
  if (h->host_out) hipHostFree(h->host_out);
  if (h->dev_noise) hipFree(h->dev_noise);
  if (h->gen_scratch) hipFree(h->gen_scratch);
  delete h;
  return MZS_OK;
}

int mzs_mlp_set_weights(mzs_handle* h, const mzs_mlp_weights* w) {
  if (!h) return MZS_E_INVALID;
  if (!w || w->struct_size != (int32_t)sizeof(mzs_mlp_weights))
    return fail(h, MZS_E_INVALID, "mzs_mlp_set_weights: null or size mismatch (ABI)");
  if (h->cfg.policy == 2)
    return fail(h, MZS_E_UNSUPPORTED, "mzs_mlp_set_weights: a stochastic handle runs the step-wise *_stochastic entries only");
  const float* const* ptrs = &w->repr_w;
  for (int i = 0; i < 18; ++i)
    if (!ptrs[i]) return fail(h, MZS_E_INVALID, "mzs_mlp_set_weights: null weight pointer");
  if (w->obs_dim <= 0 || w->support_size <= 0) return fail(h, MZS_E_INVALID, "mzs_mlp_set_weights: obs_dim/support_size");
  h->w = *w;
  h->have_weights = true;
  return MZS_OK;
}

static int register_dispatch(std::vector<mz::FusedDispatch>& list, void* dispatch, int32_t jit_abi) {
  if (!dispatch) return fail(nullptr, MZS_E_INVALID, "mzs_register_fused_dispatch: null");
  if (jit_abi != mzs_fused_jit_abi()) return fail(nullptr, MZS_E_INVALID, "mzs_register_fused_dispatch: the side library was built from other sources (ABI)");
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  for (auto f : list)
    if (reinterpret_cast<void*>(f) == dispatch) return MZS_OK;
  list.push_back(reinterpret_cast<mz::FusedDispatch>(dispatch));
  return MZS_OK;
}
int mzs_register_fused_dispatch(void* dispatch, int32_t jit_abi) { return register_dispatch(g_jit_dispatch, dispatch, jit_abi); }
int mzs_register_fused_dispatch_muzero(void* dispatch, int32_t jit_abi) {
  return register_dispatch(g_jit_dispatch_muzero, dispatch, jit_abi);
}

}  // extern "C"
