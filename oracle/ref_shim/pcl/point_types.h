/* oracle/ref_shim -- stand-in for <pcl/point_types.h> (TEST INFRASTRUCTURE, see kdtree/kdtree_flann.h).
 * Only what the reference's initRegistrationKSS.hpp and registrationMeasure.hpp touch: a point of three floats. */
#pragma once

namespace pcl {

struct PointXYZ {
    float x, y, z;
    PointXYZ() : x(0.0f), y(0.0f), z(0.0f) {}
};

}  // namespace pcl
