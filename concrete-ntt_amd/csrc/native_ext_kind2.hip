// fused external-product kernel instantiations: native kind 2
#define INST_KIND 2
#include "native_ext_inst.inc"
