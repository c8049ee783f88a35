# TEST INFRASTRUCTURE: lighting_main, a stand-alone program linked against the objects of this directory's sanitizer build (Makefile) and run directly.
# The sanitizers' runtime is linked into the program statically (the objects are the same either way), so it needs nothing from its environment.
.DEFAULT_GOAL := lighting
include $(dir $(abspath $(lastword $(MAKEFILE_LIST))))Makefile
# headers the device sources include that the Makefile's own rule for rtw_device.o does not list (see features.mk): only a build through a file that
# names them rebuilds a stale _build/rtw_device.o after an edit to one of them
$(B)/rtw_device.o: $(C)/rtw_feature_kernels.h $(C)/rtw_denoise_kernels.h $(C)/rtw_reproject_kernels.h $(C)/rtw_variance_kernels.h $(C)/rtw_upsample_kernels.h $(C)/rtw_budget_kernels.h $(C)/rtw_occlusion_kernels.h $(C)/rtw_lighting_kernels.h $(C)/rtw_tonemap_kernels.h
lighting: $(B)/lighting_main
$(B)/lighting_main: $(HERE)lighting_main.cpp $(OBJS) $(HERE)../../include/rtwin.h
	$(CXX) $(filter-out -shared-libasan,$(FLAGS)) -I$(HERE)../../include $< $(OBJS) -o $@ -lz -lpthread -ldl
