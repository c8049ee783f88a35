# TEST INFRASTRUCTURE: features_main, a stand-alone program linked against the objects of this directory's sanitizer build (Makefile) and run directly.
# The sanitizers' runtime is linked into the program statically (the objects are the same either way), so it needs nothing from its environment.
.DEFAULT_GOAL := features
include $(dir $(abspath $(lastword $(MAKEFILE_LIST))))Makefile
# the device sources include the feature kernels' header, which the Makefile's own list of them predates.  Only a build through THIS file knows it:
# Makefile itself and camera.mk / lens.mk / material.mk / query.mk reuse a stale _build/rtw_device.o after an edit to that header (make clean first);
# the next change that may touch Makefile should add the header to its rtw_device.o rule and drop this line
$(B)/rtw_device.o: $(C)/rtw_feature_kernels.h
features: $(B)/features_main
$(B)/features_main: $(HERE)features_main.cpp $(OBJS) $(HERE)../../include/rtwin.h
	$(CXX) $(filter-out -shared-libasan,$(FLAGS)) -I$(HERE)../../include $< $(OBJS) -o $@ -lz -lpthread -ldl
