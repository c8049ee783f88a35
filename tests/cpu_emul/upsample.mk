# TEST INFRASTRUCTURE: upsample_main, a stand-alone program linked against the objects of this directory's sanitizer build (Makefile) and run directly.
# The sanitizers' runtime is linked into the program statically (the objects are the same either way), so it needs nothing from its environment.
.DEFAULT_GOAL := upsample
include $(dir $(abspath $(lastword $(MAKEFILE_LIST))))Makefile
# the device sources include these headers, which the Makefile's own list of them predates (see features.mk)
$(B)/rtw_device.o: $(C)/rtw_feature_kernels.h $(C)/rtw_denoise_kernels.h $(C)/rtw_reproject_kernels.h $(C)/rtw_variance_kernels.h $(C)/rtw_upsample_kernels.h
upsample: $(B)/upsample_main
$(B)/upsample_main: $(HERE)upsample_main.cpp $(OBJS) $(HERE)../../include/rtwin.h
	$(CXX) $(filter-out -shared-libasan,$(FLAGS)) -I$(HERE)../../include $< $(OBJS) -o $@ -lz -lpthread -ldl
