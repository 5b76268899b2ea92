// Plain views of the two MCTS networks for a translation unit that reads their parameters in
// place (mcts_search.hip): the bound parameter pointer, the shapes and where every tensor
// starts in the flat buffer (offsets in floats).  az.hip and mlp_model.hip each fill their own.
#pragma once

#include <cstdint>

#include "acme_hip.h"

namespace acme {

// acme_az: trunk layer i is sizes[i - 1] (obs_dim for i = 0) -> sizes[i], then the two heads.
struct AzView {
  const float* params;  // null before acme_az_bind
  int64_t flat;
  int obs_dim, num_actions, nl, relu_final;
  int sizes[ACME_MAX_MLP_LAYERS];
  int w[ACME_MAX_MLP_LAYERS], b[ACME_MAX_MLP_LAYERS];
  int pw, pb, vw, vb;
};

// acme_mlp_model: tower t (state, reward, discount logit), linear layer j is
// width[t][j] -> width[t][j + 1]; width[t][0] = obs_dim + num_actions.
struct MlpModelView {
  const float* params;  // null before acme_mlp_model_bind
  int64_t flat;
  int obs_dim, num_actions, L;
  int width[3][ACME_MLP_MODEL_MAX_HIDDEN + 2];
  int woff[3][ACME_MLP_MODEL_MAX_HIDDEN + 1], boff[3][ACME_MLP_MODEL_MAX_HIDDEN + 1];
};

void az_view(const acme_az* l, AzView* out);
void mlp_model_view(const acme_mlp_model* l, MlpModelView* out);

}  // namespace acme
