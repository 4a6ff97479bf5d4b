// pnvo_policy_state.h — the navigation policy's handle, shared by its per-step forward (pnvo_policy.hip) and its PPO update step
// (policy_train.hip).
#pragma once
#include <vector>

#include "../../include/pnvo.h"

namespace pnvo {

struct PolicyTrain;                  // policy_train.hip: flat-buffer offsets, saved activations and scratch of the update step

struct Policy {
  pnvo_policy_config cfg;
  int device = 0;
  pnvo_handle enc = nullptr;
  bool loaded = false;
  // device weights (torch layouts): owned copies, or — once a train step is attached — pointers into the caller's flat buffer
  float *emb = nullptr, *tgt_w = nullptr, *tgt_b = nullptr;
  std::vector<float *> w_ih, w_hh, b_ih, b_hh;
  float *act_w = nullptr, *act_b = nullptr, *cr_w = nullptr, *cr_b = nullptr;
  bool attached = false;             // pnvo_policy_train_attach: the weight pointers above are not owned
  PolicyTrain *train = nullptr;
  // workspace
  int cap = 0;
  float *pooled = nullptr, *visual = nullptr, *x = nullptr;
};

void pnvo_policy_free_weights(Policy &p);     // pnvo_policy.hip: frees the owned copies (no-op on borrowed pointers) and nulls them
void pnvo_policy_train_free(Policy &p);       // policy_train.hip

}  // namespace pnvo

extern "C" {
struct pnvo_policy_s {
  pnvo::Policy p;
};
}
