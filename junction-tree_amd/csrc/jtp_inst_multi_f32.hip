// One family of message-passing kernels for one storage type, compiled on its own: its bodies are jtp_k_multi.h, its list is in jtp_kernels.hip.h ("Explicit instantiation lists").
#define JT_INST_TU
#include "jtp_k_multi.h"
JT_INST_MULTI(, float)
