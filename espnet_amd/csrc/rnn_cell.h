// espnet_amd — the recurrent cells of torch.nn.LSTM / torch.nn.GRU on summed gate pre-activations (f32), shared by the
// SequentialRNNLM step (csrc/search.hip rnn_cell_kernel) and the transducer's prediction network (csrc/transducer.hip):
// one implementation of the cell arithmetic.
#pragma once
#include "em_common.h"

// LSTM, gates i | f | g | o:  c' = s(f) c + s(i) tanh(g),  h' = s(o) tanh(c').  Returns h', *c_new = c'.
__device__ __forceinline__ float em_lstm_cell(float pi, float pf, float pg, float po, float c_prev, float* c_new) {
  const float gi = 1.f / (1.f + expf(-pi)), gf = 1.f / (1.f + expf(-pf));
  const float gg = tanhf(pg), go = 1.f / (1.f + expf(-po));
  const float cc = gf * c_prev + gi * gg;
  *c_new = cc;
  return go * tanhf(cc);
}

// GRU, gates r | z | n_x | n_h (EmRnnLayer):  n = tanh(n_x + s(r) n_h),  h' = (1 - s(z)) n + s(z) h.
__device__ __forceinline__ float em_gru_cell(float pr, float pz, float pnx, float pnh, float h_prev) {
  const float gr = 1.f / (1.f + expf(-pr)), gz = 1.f / (1.f + expf(-pz));
  const float nn = tanhf(pnx + gr * pnh);
  return (1.f - gz) * nn + gz * h_prev;
}
