/* oracle/ref_shim -- empty stand-in for <pcl/io/pcd_io.h>: the reference's initRegistrationKSS.hpp includes it
 * and uses nothing from it (see kdtree/kdtree_flann.h). */
#pragma once
