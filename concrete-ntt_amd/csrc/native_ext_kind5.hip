// fused external-product kernel instantiations: native kind 5
#define INST_KIND 5
#include "native_ext_inst.inc"
