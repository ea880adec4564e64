// fused external-product kernel instantiations: native kind 4
#define INST_KIND 4
#include "native_ext_inst.inc"
