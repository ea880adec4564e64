// fused decomposing external-product kernel instantiations: native kind 3
#define INST_KIND 3
#include "native_gadget_inst.inc"
